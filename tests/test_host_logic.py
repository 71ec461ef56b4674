"""CPU tests of the host logic: sharding, the world_size-2 gloo collectives, the C-ABI symbol
table, the oracle/product separation, and loud failure without a GPU."""
import glob
import os
import re
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_bounds_cover_everything_exactly_once():
    from rald_amd.distributed import shard_bounds, shard_sample_indices
    for total in (0, 1, 7, 8, 64, 1000003):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    # DistributedSampler-style interleave: every sample appears, ranks get equal counts
    for total, world in ((10, 4), (8, 8), (3, 8)):
        per = [shard_sample_indices(total, r, world) for r in range(world)]
        assert len({len(p) for p in per}) == 1
        assert set(sum(per, [])) == set(range(total))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from rald_amd import distributed as D
    r, w, _ = D.init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    # per-rank shard of 5 independent samples, each "metric" = its global index
    lo, hi = D.shard_bounds(5, rank, world)
    total, count = D.reduce_sum_count(float(sum(range(lo, hi))), float(hi - lo))
    mx = D.max_over_ranks(1.0 + rank)
    mean = D.all_reduce_mean(float(rank))
    local = torch.arange(lo, hi, dtype=torch.float32).reshape(-1, 1) * torch.ones(1, 3)
    gathered = D.gather_shards(local, [b - a for a, b in (D.shard_bounds(5, rr, world) for rr in range(world))])
    q.put((rank, total, count, mx, mean, None if gathered is None else gathered[:, 0].tolist()))
    torch.distributed.destroy_process_group()


def test_world_size_2_gloo_collectives():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, total, count, mx, mean, gathered in res:
        assert total == 10.0 and count == 5.0          # 0+1+2+3+4 over both shards
        assert mx == 2.0 and abs(mean - 0.5) < 1e-6
    assert res[0][5] == [0.0, 1.0, 2.0, 3.0, 4.0] and res[1][5] is None


class _FakeVae:
    """decode = a deterministic function of the queries alone (what the real decoder is, given z)."""
    calls = 0

    def decode(self, z, queries):
        _FakeVae.calls += 1
        return (queries * torch.tensor([1.0, -2.0, 0.5])).sum(-1, keepdim=True) + z.sum()


def _qsplit_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from rald_amd import distributed as D, synth
    D.init_distributed(backend="gloo")
    z = torch.ones(1, 4, 2)
    out = {}
    for Q in (1001, 2, 1, 0):                                   # ragged, Q == world, Q < world, empty
        queries = synth.queries(1, Q, seed=90) if Q else torch.zeros(1, 0, 3)
        out[Q] = D.decode_queries_sharded(_FakeVae(), z, queries)
    q.put((rank, {k: v.numpy() for k, v in out.items()}, _FakeVae.calls))
    torch.distributed.destroy_process_group()


def test_query_sharded_decode_gloo_world2():
    """SURVEY.md §8e second-level split: each rank decodes a slice of one sample's queries, all ranks end with all logits."""
    from rald_amd import synth
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_qsplit_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    vae, z = _FakeVae(), torch.ones(1, 4, 2)
    for rank, outs, calls in res:
        for Q, got in outs.items():
            queries = synth.queries(1, Q, seed=90) if Q else torch.zeros(1, 0, 3)
            want = vae.decode(z, queries).numpy()
            assert got.shape == (1, Q, 1) and (got == want).all()
    assert res[0][2] == 3 and res[1][2] == 2                    # rank 1 has no queries at Q = 1; nobody decodes at Q = 0


def test_c_abi_library_loads_and_exports_every_declared_symbol():
    """Every function include/rald_hip.h declares must be exported by librald_hip.so and bound in
    rald_amd._lib.SIGNATURES (no compute calls here: there is no GPU)."""
    from rald_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rald_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rald_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 25
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in rald_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is res and tuple(fn.argtypes) == tuple(args), name
    assert L.rald_version() >= 1


def test_c_abi_signatures_are_derived_from_the_header():
    """_lib reads restype / argtypes off the header's prototypes: scalars keep their width, every pointer is a c_void_p."""
    import ctypes as C
    from rald_amd import _lib
    P, I32, I64, F, D = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    S = _lib.SIGNATURES
    assert S["rald_optim_adamw_ema"] == (I32, [P, P, P, P, P, I64, P, D, D, D, D, D, I64, D, I32, P])
    assert S["rald_dit_profile_set_kinds"] == (I32, [P, C.c_uint32])
    assert S["rald_last_error"] == (C.c_char_p, [])
    assert S["rald_dit_destroy"] == (None, [P])
    assert S["rald_lidar_create"] == (I32, [P, P])                                 # const rald_lidar_config*, rald_lidar**
    assert S["rald_debug_f16_saturation_count"] == (I64, [I32])
    assert S["rald_dit_sample"] == (I32, [P, P, I32, P, I32, F, F, F, P, P])
    assert S["rald_op_ae_encode_tables"] == (I32, [I32, I32, I32, I32, P, P])       # const float* const*, float* const*
    assert len(S["rald_op_attention_bwd"][1]) == 32
    assert S["rald_op_resid_gemm_ln"] == (I32, [P, P, P, I64, P, P, P, I64, I64, I32, P, P, P, P, P, P, P, I64, I32, F, F, I32, I32, I32, I32, P, I64, P])
    assert S["rald_op_attention_args"] == (I32, [P, P, I64, I64, P, I64, I64, I32, P, I64, I64, P, I64, I64, P, I64, I64, I32, I32, I32, I32, F, I32, I32,
                                                 I32, I32, I32, P, I64, P])
    assert S["rald_op_attn_self_proj_slabs"] == (I32, [P, I64, P, P, I32, I32, I32, I32, P])
    assert S["rald_op_xattn_q2_proj_slabs"] == (I32, [P, P, P, I64, I64, P, I64, I64, P, P, I32, I32, I32, I32, F, I32, P])
    assert S["rald_op_reduce_resid_ln_slabs"] == (I32, [P, I32, I64, P, P, P, I32, P, P, I64, I32, F, F, I32, P])
    assert S["rald_debug_f16_saturation_attn"] == (I64, [I32]) and S["rald_op_attention_pick_ksplit"] == (I32, [I32, I32, I32, I32])
    assert S["rald_op_gemm_geglu_mx8out"] == (I32, [P, P, P, I64, P, P, P, I64, P, P, P, P, I64, I32, I32, I32, P])


def test_c_abi_unknown_type_is_refused_at_load(tmp_path):
    from rald_amd import _lib
    h = tmp_path / "h.h"
    h.write_text("/* size_t is not part of the ABI */\nint rald_ok(int32_t a, const float* b);\nint rald_bad(int32_t a, size_t n);\n")
    with pytest.raises(RuntimeError, match=r"size_t.*rald_bad"):
        _lib._parse(str(h))


def test_c_abi_config_structs_match_the_header_layout():
    """sizeof and field offsets of the five config structs, worked out by hand from include/rald_hip.h."""
    import ctypes as C
    from rald_amd import _lib
    off = lambda S: {name: getattr(S, name).offset for name, _ in S._fields_}
    dit = ["n_latents", "channels", "depth", "n_heads", "d_head", "t_channels", "context_dim", "n_cond_tokens", "with_radar_enc",
           "enc_hidden_ch", "enc_radar_ch", "radar_r", "radar_a", "radar_e", "sigma_data", "qkv_dtype"]
    assert C.sizeof(_lib.DitConfig) == 64 and off(_lib.DitConfig) == {n: 4 * i for i, n in enumerate(dit)}
    assert _lib.DitConfig.sigma_data.size == 4 and _lib.DitConfig._fields_[14][1] is C.c_float
    ae = ["dim", "num_latents", "latent_dim", "depth", "heads", "dim_head", "num_inputs", "query_type"]
    assert C.sizeof(_lib.AeConfig) == 32 and off(_lib.AeConfig) == {n: 4 * i for i, n in enumerate(ae)}
    dsp = ["ntx", "nrx", "n_chirps", "n_samples", "range_fft", "doppler_fft", "angle_fft", "elevation_fft"]
    assert C.sizeof(_lib.RadarDspConfig) == 48
    assert off(_lib.RadarDspConfig) == {**{n: 4 * i for i, n in enumerate(dsp)}, "crop_low": 32, "crop_high": 40}
    pts = ["in_r", "in_a", "in_e", "in_channels", "tgt_r", "tgt_a", "tgt_e"]
    assert C.sizeof(_lib.RadarPointsConfig) == 40
    assert off(_lib.RadarPointsConfig) == {**{n: 4 * i for i, n in enumerate(pts)}, "num_points": 32}      # int64_t after 4 bytes of padding
    assert _lib.RadarPointsConfig.num_points.size == 8
    lid = ["max_points_per_voxel", "max_voxels", "num_point_features", "view_cone_mode", "norm_anisotropy", "norm_isotropy"]
    assert C.sizeof(_lib.LidarConfig) == 272
    assert off(_lib.LidarConfig) == {"pc_range": 0, "voxel_size": 48, **{n: 72 + 4 * i for i, n in enumerate(lid)}, "extrinsic": 96, "fov": 224}
    assert (_lib.LidarConfig.pc_range.size, _lib.LidarConfig.extrinsic.size, _lib.LidarConfig.fov.size) == (48, 128, 48)


def test_errors_are_reported_not_crashed():
    import ctypes as C
    from rald_amd import _lib
    L = _lib.lib()
    cfg = _lib.DitConfig()
    L.rald_dit_default_config(C.byref(cfg))
    assert (cfg.n_latents, cfg.channels, cfg.depth, cfg.context_dim) == (512, 32, 24, 512)
    rc = L.rald_dit_create(None, None)
    assert rc != 0 and b"null" in L.rald_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc)


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under rald_amd/ may import, call or link it."""
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|rald_oracle", re.M)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rald_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not pat.search(src), f"{f} references the oracle"


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a GPU-less box")
def test_cpu_tensors_fail_loudly_no_fallback():
    from rald_amd import models_ae as A, models_radar_generation as G
    m = G.LatentArrayTransformer(in_channels=32, t_channels=256, n_heads=8, d_head=64, depth=1)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 512, 32), torch.tensor([0.1]), cond=torch.zeros(1, 64, 512))
    ae = A.create_autoencoder(dim=256, M=128, latent_dim=32, N=1000, query_type="mix")
    with pytest.raises(RuntimeError):
        ae.encode(torch.zeros(1, 1000, 3))


def test_factories_and_unsupported_paths():
    from rald_amd import config, models_ae as A, models_radar_generation as G
    cfg = config.shipped_generation_config()
    for name in ("kl_d512_m512_l8_edm", "kl_d512_m512_l16_edm", "kl_d512_m512_l32_edm", "kl_d512_m512_l4_d24_edm",
                 "kl_d512_m512_l8_d24_edm", "kl_d512_m512_l32_d18_edm", "kl_d512_m512_l32_d12_edm"):
        assert callable(G.__dict__[name])
    m = G.__dict__["kl_d512_m512_l32_d12_edm"](configs=cfg)
    assert m.depth == 12 and m.channels == 32 and m.model.proj_out.weight.abs().max() == 0   # zero-init (:198-201)
    with pytest.raises(NotImplementedError):
        A.kl_d512_m512_l32(N=2048)                    # query_type='point' needs torch_cluster.fps
    ae = A.__dict__["kl_d512_m512_l32_mix"](N=10000)
    assert ae.num_inputs == 10000 and ae.latent_dim == 32
    with pytest.raises(NotImplementedError):
        G.edm_sampler(m, torch.zeros(1, 512, 32), None, "radar", S_churn=1)


def test_documented_import_swap_resolves():
    """the reference's model-layer import lines (main_generation.py:22, engine_generation.py:25-27,
    main_ae.py:21, engine_ae.py:16, main_cache.py:17 - restated here as the interface contract) with `model` replaced by
    `rald_amd` must import, and the names the engines use in isinstance / __dict__ lookups must be the package's classes."""
    import re
    lines = ["from model import models_ae, models_radar_encoder, models_radar_generation",      # main_generation.py:22
             "from model.models_ae import  KLAutoEncoder",                                        # engine_generation.py:25, engine_ae.py:16
             "from model.models_radar_encoder import RadarAutoencoder",                           # engine_generation.py:26
             "from model.models_radar_generation import EDMPrecond, EDMLoss",                     # engine_generation.py:27
             "from model import models_ae"]                                                       # main_ae.py:21, main_cache.py:17
    ns = {}
    for ln in lines:
        exec(re.sub(r"\bmodel\b", "rald_amd", ln), ns)
    import rald_amd
    assert ns["models_ae"] is rald_amd.models_ae and ns["KLAutoEncoder"] is rald_amd.models_ae.KLAutoEncoder
    assert ns["EDMPrecond"] is rald_amd.models_radar_generation.EDMPrecond and callable(ns["EDMLoss"])
    assert ns["RadarAutoencoder"] is rald_amd.models_radar_encoder.RadarAutoencoder
    # the factory lookups of main_generation.py:110, :122, :134, :164 and main_ae.py
    for mod, names in ((ns["models_ae"], ["kl_d512_m512_l32_mix", "kl_d512_m512_l32_learn"]),
                       (ns["models_radar_generation"], ["kl_d512_m512_l32_d24_edm", "EDMLoss"]),
                       (ns["models_radar_encoder"], ["ae_ch64_mult5_n2_d16"])):
        for n in names:
            assert callable(mod.__dict__[n]), n


def test_shipped_library_reads_no_environment_variable():
    """The library has no run-time A/B or ablation switches: it must not even import getenv, its sources must not name it,
    and it must report build flags 0."""
    import subprocess
    from rald_amd import _lib
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in und
    assert _lib.lib().rald_build_flags() == 0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "rald_amd", "csrc")
    srcs = [os.path.join(csrc, "Makefile")] + glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")) + \
        glob.glob(os.path.join(root, "include", "*.h"))
    assert srcs
    for path in srcs:
        with open(path) as f:
            text = f.read()
        for word in ("getenv", "RALD_PROBE", "RALD_ABLATED"):
            assert word not in text, (path, word)
    # one form per kernel: no compile-time variants in the shipped sources (only the host / device split of kernels.h)
    kernel_srcs = glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip"))
    for path in kernel_srcs:
        with open(path) as f:
            for n, line in enumerate(f, 1):
                m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif|elifdef|elifndef)\b(.*)", line)
                if m:
                    cond = m.group(2).split("//")[0]
                    assert "RALD_" not in cond, (path, n, line)
                    names = set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
                    assert names == {"__HIPCC__"}, (path, n, line)
    # and no tool compiles a variant of them: nothing under tools/ includes a product source
    product = {os.path.basename(p) for p in kernel_srcs}
    tools = [p for p in glob.glob(os.path.join(root, "tools", "**", "*"), recursive=True) if os.path.isfile(p)]
    assert tools
    for path in tools:
        with open(path, errors="replace") as f:
            for n, line in enumerate(f, 1):
                m = re.match(r'\s*#\s*include\s*[<"]([^>"]+)[>"]', line)
                if m:
                    inc = m.group(1)
                    assert "csrc" not in inc and os.path.basename(inc) not in product, (path, n, line)


def test_each_op_entry_point_is_called_from_one_module():
    """A rald_op_* entry point has one Python wrapper: it is called from one module of the package only (the three trainers share the
    wrappers of train_ops.py), and an optional argument is a nullable parameter of the entry, not a second entry beside it."""
    callers = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "rald_amd", "*.py"))):
        with open(path) as f:
            for name in set(re.findall(r"\.(rald_op_\w+)\s*\(", f.read())):
                callers.setdefault(name, []).append(os.path.basename(path))
    shared = {name: mods for name, mods in callers.items() if len(mods) > 1}
    assert not shared, shared
    with open(os.path.join(ROOT, "include", "rald_hip.h")) as f:
        hdr = f.read()
    # (kept entry, suffix of the twin it absorbed)
    for kept, suffix in (("rald_op_gemm_tn", "_ws"), ("rald_op_conv3d_wgrad", "_ws"), ("rald_op_ln_mod_bwd", "_cast"), ("rald_op_groupnorm_bwd", "_cast"),
                         ("rald_op_conv3d", "_bf16")):
        assert re.search(rf"\b{kept}\s*\(", hdr) and not re.search(rf"\b{kept}{suffix}\b", hdr), kept + suffix


def test_module_forward_checks_batch_sizes_before_touching_the_gpu():
    """a condition batch that does not match x used to reach the kernels (out-of-bounds reads)."""
    from rald_amd import models_radar_generation as G
    m = G.LatentArrayTransformer(in_channels=32, t_channels=256, n_heads=8, d_head=64, depth=1)
    with pytest.raises(RuntimeError, match="one set of condition tokens per sample"):
        m(torch.zeros(3, 512, 32), torch.tensor([0.1]), cond=torch.zeros(2, 64, 512))
    with pytest.raises(RuntimeError, match="channels"):
        m(torch.zeros(2, 512, 16), torch.tensor([0.1]), cond=torch.zeros(2, 64, 512))


def test_training_workspace_queries_are_host_side_and_consistent():
    """The workspace / scratch sizes of the atomic-free gradient kernels are plain host arithmetic (no GPU needed): they grow with the number of
    row / voxel ranges, cover at least one range of the full gradient, are 0 where a shape keeps the atomic form, and refuse nonsense."""
    from rald_amd._lib import lib
    L = lib()
    # Linear weight gradient dW [N1, N2] over M rows: (ranges) x (N1*N2 + N1) floats
    b = L.rald_op_gemm_tn_workspace_bytes(4096, 4096, 512)
    assert b >= 4 * (4096 * 512 + 4096) and b % (4 * (4096 * 512 + 4096)) == 0
    assert L.rald_op_gemm_tn_workspace_bytes(4096, 64, 512) == 0             # narrow outputs keep their atomics
    assert L.rald_op_gemm_tn_workspace_bytes(0, 512, 512) == 0
    # Conv3d weight gradient at the radar encoder's levels (B = 8): per range Cout*27*Cin + Cout floats
    for (D, H, W, Cin, Cout) in ((128, 64, 32, 64, 64), (32, 16, 8, 128, 128), (8, 4, 2, 256, 256)):
        b = L.rald_op_conv3d_wgrad_workspace_bytes(8, D, H, W, Cin, Cout, 1, 1)
        per = 4 * (Cout * 27 * Cin + Cout)
        assert b >= per and b % per == 0, (D, H, W, Cin, Cout, b)
    assert L.rald_op_conv3d_wgrad_workspace_bytes(8, 128, 64, 32, 64, 64, 3, 1) == 0      # unsupported stride
    # GroupNorm backward scratch: group sums + one row of partial sums per 1 024 voxels and sample + per-sample channel sums
    B, S, C = 8, 128 * 64 * 32, 64
    nblk = (S + 1023) // 1024
    assert L.rald_op_groupnorm_bwd_scratch_bytes(B, S, C) == B * 64 * 8 + (B * nblk * (2 * C + 64) + B * 2 * C) * 4
    assert L.rald_op_groupnorm_bwd_scratch_bytes(0, S, C) == 0
