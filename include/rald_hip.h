/* rald_hip.h - C-ABI of librald_hip.so: the MI355X (gfx950) implementation of RaLD's hot path.
 *
 * The reference (RoyAPTX4869/RaLD) has no FFI of its own: its seam is the Python nn.Module API
 * (SURVEY.md 8b).  These entry points are what a binding for that seam calls; each one names
 * the reference interface (file:line under the reference root) it replaces.  INTEGRATION.md
 * shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; rald_last_error() gives the
 *     message for the calling thread.  Nothing is printed, nothing aborts.
 *   - all tensor pointers are DEVICE pointers (hipMalloc'd or torch-allocated), dense,
 *     row-major, fp32 unless stated; `stream` is a hipStream_t (NULL = default stream).
 *     Work is enqueued on `stream`; no entry point synchronises except *_create / *_destroy /
 *     *_load_weight / *_finalize / *_reserve (setup-time, blocking).
 *   - handles are re-entrant per handle (one stream at a time per handle); no global state.
 *   - weights are loaded by their reference checkpoint key (utils/misc.py:309-316), fp32,
 *     from host OR device memory; packing to the kernels' layouts (bf16, fused/permuted rows)
 *     happens inside the library.
 */
#ifndef RALD_HIP_H
#define RALD_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* rald_last_error(void);
int rald_version(void);
/* Always 0: the library reads no environment variable and has no work-skipping build.  bench.py refuses to measure a
 * library that reports anything else. */
int rald_build_flags(void);
/* Diagnostic (synchronises the device): how many times a lane clamped a value while writing an fp16 partial-sum slab since the last
 * reset.  The small-batch paths (<= 2 samples) pass per-head / split-K partial sums between kernels as fp16 x 2^-6, saturating at
 * +-4.19e6; a non-zero count means a result was clipped.  Returns -1 on a HIP error. */
int64_t rald_debug_f16_saturation_count(int32_t reset);
/* Diagnostic: one launch that leaves all 160 KiB of LDS of every CU filled with NaN patterns (0x7fc07fc0).  LDS is not cleared
 * between workgroups, so a kernel that reads a word it never wrote is only wrong when something else ran on that CU before it -
 * i.e. under concurrent streams.  The test suite poisons the LDS and requires bit-identical results. */
int rald_debug_poison_lds(void* stream);

/* ------------------------------------------------------------------------------------------
 * Denoiser: EDMPrecond + LatentArrayTransformer  (model/models_radar_generation.py:171-233,
 * :314-449)
 * ---------------------------------------------------------------------------------------- */
typedef struct rald_dit rald_dit;

typedef struct rald_dit_config {
    int32_t n_latents;      /* 512  (EDMPrecond n_latents, :316)                        */
    int32_t channels;       /* 32   latent channels C (:317)                            */
    int32_t depth;          /* 24   transformer blocks (:324, factories :452-482)       */
    int32_t n_heads;        /* 8                                                        */
    int32_t d_head;         /* 64   (only 64 is implemented)                            */
    int32_t t_channels;     /* 256  PositionalEmbedding width (:336)                    */
    int32_t context_dim;    /* 512  width of the condition tokens (:180-193)            */
    int32_t n_cond_tokens;  /* 64   = 8*4*2 radar tokens (:405)                         */
    int32_t with_radar_enc; /* 1: radar_enc.* / radar_*_emb / radar_token_project loaded */
    int32_t enc_hidden_ch;  /* 64   (configs.enc_hidden_ch, :348)                       */
    int32_t enc_radar_ch;   /* 16   (configs.enc_radar_ch, :349)                        */
    int32_t radar_r, radar_a, radar_e; /* 128, 64, 32 input cube (R,A,E)                */
    float sigma_data;       /* 1.0 (:321)                                               */
    int32_t qkv_dtype;      /* 0 = bf16 (default); 1 = MXFP8 e4m3 for the attention q/k/v projections (BASELINE config #5); 2 = also the GEGLU projection; 3 = also ff.net.2 */
} rald_dit_config;

void rald_dit_default_config(rald_dit_config* cfg);
int rald_dit_create(const rald_dit_config* cfg, rald_dit** out);
void rald_dit_destroy(rald_dit* h);
/* One tensor of the reference state_dict, by key (e.g. "model.transformer_blocks.3.attn1.to_q.weight");
 * `data` = fp32, host or device, `nelem` elements.  Unknown keys and wrong sizes are errors. */
int rald_dit_load_weight(rald_dit* h, const char* name, const float* data, int64_t nelem);
/* Checks that every key was loaded (strict=True semantics, utils/misc.py:346). */
int rald_dit_finalize(rald_dit* h);
/* Pre-allocates activation workspace for batches up to max_batch (otherwise grown on demand). */
int rald_dit_reserve(rald_dit* h, int32_t max_batch);
/* Counts the reallocations of handle-owned device buffers (activation workspace, noise-level tables).  A caller that
 * captured library calls into a hipGraph must re-capture when the value differs from the one read after capture: the
 * graph's kernels hold pointers into those buffers. */
int64_t rald_dit_workspace_generation(const rald_dit* h);
/* Two-stream schedule of an NFE (rald_dit_denoise / rald_dit_sample): from `min_batch` samples up (default 256; measured: +1.9 % there,
 * nothing at 128) the batch runs as
 * two half-batches on two HIP streams - the caller's and a handle-owned one, forked from and joined back into `stream` with events,
 * so the caller sees ordinary stream semantics.  Every CU of one launch runs the same phase at the same time (matrix loop, then the
 * store-heavy epilogue); a second independent half-batch fills those holes.  Each half runs exactly the kernels a batch of its size
 * runs alone: results are bit-identical to two sequential calls.  0 = never split.  Re-plans the workspace (blocking). */
int rald_dit_set_two_stream_min_batch(rald_dit* h, int32_t min_batch);
int32_t rald_dit_two_stream_min_batch(const rald_dit* h);

/* Noise-level table: for each of the n sigmas (HOST array) computes the EDM coefficients
 * (c_in, c_skip, c_out, c_noise; :422-425), the timestep embedding (:217-219) and all
 * depth*3 AdaLayerNorm modulations (:128-129) once; rald_dit_denoise refers to rows of it. */
int rald_dit_set_sigmas(rald_dit* h, const float* sigmas_host, int32_t n, void* stream);

/* Bytes of the condition cache FOR THIS BATCH SIZE (a cache is built for, and used with, one batch size; it starts with a 64-byte
 * header - magic, batch, layout flag, configuration hash - that rald_dit_denoise / rald_dit_sample check against their `batch`
 * argument BEFORE any launch: a cache this handle has not seen (a copy) is verified once by reading the header back, which
 * synchronises `stream` and cannot happen under graph capture): K and V^T of the condition
 * tokens for every block, and from 3 samples up (bf16 mode) also the folded forms K.to_q and to_out.V^T per sample and block
 * (1 MiB each) that turn the cross-attention sub-block into two GEMMs - not a linear function of `batch`, so always ask. */
int64_t rald_dit_cond_cache_bytes(const rald_dit* h, int32_t batch);
/* Condition tokens [B, n_cond_tokens, context_dim] -> cond cache (the K/V projections of
 * attn2 are step-invariant; CrossAttention.to_k/to_v :63-64). */
int rald_dit_encode_cond_tokens(rald_dit* h, const float* tokens, int32_t batch, void* cond_cache, void* stream);
/* EDMPrecond.process_radar_cond (:363-407): cube [B,R,A,E,2] -> tokens [B,64,C] (optional
 * output, may be NULL) and the cond cache.  Run ONCE per sample, outside the sampling loop. */
int rald_dit_encode_cond(rald_dit* h, const float* cube, int32_t batch, float* out_tokens, void* cond_cache, void* stream);

/* One NFE = EDMPrecond.forward (:412-430) with the condition already encoded:
 *   D_x = c_skip*x + c_out*F(c_in*x, c_noise, cond).   x,out: [B, n_latents, channels].
 * sigma_row selects the row of the table set by rald_dit_set_sigmas; per_sample != 0 means
 * sample b uses row sigma_row+b (training-style [B,1,1] sigmas, :419).
 * raw_F != 0 returns F(x, c_noise, cond) with no pre/post-conditioning
 * (= LatentArrayTransformer.forward, :215-233, c_noise = ln(sigma)/4 of the table row). */
int rald_dit_denoise(rald_dit* h, const float* x, int32_t batch, int32_t sigma_row, int32_t per_sample,
                     const void* cond_cache, float* out, int32_t raw_F, void* stream);

/* edm_sampler (:235-275) at S_churn=0: latents [B,n_latents,channels] ~ N(0,1) -> samples.
 * 2*num_steps-1 NFEs.  The sigma table is (re)built internally for the schedule. */
int rald_dit_sample(rald_dit* h, const float* latents, int32_t batch, const void* cond_cache, int32_t num_steps,
                    float sigma_min, float sigma_max, float rho, float* out, void* stream);

/* The noise levels of edm_sampler (:246-249, :258-259) on the HOST, fp32 in the reference's operation order: the Karras levels
 * t [num_steps + 1] (t_N = 0) and t_hat [num_steps], t_hat_i = t_i + gamma * t_i with gamma = min(S_churn / num_steps, sqrt(2) - 1)
 * where S_min <= t_i <= S_max, else 0.  Step i is CHURNED iff t_hat[i] != t[i].  rald_dit_sample_stochastic uses this function; a
 * caller asks it which steps need noise.  Needs no GPU.  The scalars are doubles because the reference evaluates sigma^(1/rho) and
 * S_churn / num_steps as Python floats before they meet fp32 tensors; t agrees with the reference's t_steps bit for bit on the shipped
 * schedule (rald_dit_sample's own all-fp32 table differs from it by a few ulp and is left as it is). */
int rald_edm_schedule(int32_t num_steps, double sigma_min, double sigma_max, double rho, double S_churn, double S_min, double S_max, float* t,
                      float* t_hat);
/* edm_sampler (:235-275) with S_churn >= 0.  Before the Euler NFE of every churned step i the state is raised to t_hat_i,
 *   x_hat = x + sqrt(t_hat_i^2 - t_i^2) * S_noise * n_i,
 * with n_i read from `noise` - [n_churned, B, n_latents, channels], the churned steps only, in step order - or generated in the
 * same kernel from `seeds` (int64 [B], device; rald_op_philox_normal's stream with tag 1 and step = i).  Exactly one of the two is
 * non-NULL when a step is churned.  With no churned step this IS rald_dit_sample (same kernels, same bits; noise / seeds ignored).
 * Enqueues only (no allocation or synchronisation once the batch and the schedule have been seen): the call captures into a hipGraph. */
int rald_dit_sample_stochastic(rald_dit* h, const float* latents, int32_t batch, const void* cond_cache, int32_t num_steps, double sigma_min,
                               double sigma_max, double rho, double S_churn, double S_min, double S_max, double S_noise, const float* noise,
                               const int64_t* seeds, float* out, void* stream);
/* Counter-based N(0,1) on the device: out [B, n_per_sample] (16-byte aligned; n_per_sample a multiple of 4), a pure function of
 * (seed, tag, step, element).  Philox4x32-10 with key (seeds[b] mod 2^32, tag) and counter (e / 4, step, 0, 0) gives elements
 * 4*(e/4) .. +3 by Box-Muller: u1 = ((x >> 8) + 1) * 2^-24, u2 = (y >> 8) * 2^-24, r = sqrtf(-2 logf(u1)), (r cosf(2 pi u2),
 * r sinf(2 pi u2)) from the word pairs (x0, x1) and (x2, x3).  tag 0 = initial latents, 1 = churn noise.  seeds: int64 [B], device. */
int rald_op_philox_normal(const int64_t* seeds, int32_t B, int64_t n_per_sample, int32_t tag, int32_t step, float* out, void* stream);

/* Live timing of the dominant kernel (the FF1 GEGLU GEMM, FeedForward :88-117): between begin
 * and end every launch of it inside rald_dit_denoise is bracketed by HIP events recorded on the
 * launch stream (up to 4096 launches); end synchronises those events and returns their sum. */
int rald_dit_profile_begin(rald_dit* h);
int rald_dit_profile_end(rald_dit* h, double* total_ms, int32_t* launches);
/* The same bracket also times the three fused residual + LayerNorm GEMMs of a block (the largest time share of an NFE); this form
 * returns all four kinds: [0] FF1 GEGLU GEMM, [1] attn1.to_out + residual + AdaLN (K = 512), [2] attn2 output projection + residual
 * + AdaLN (K = 512), [3] ff.net.2 + residual + AdaLN (K = 2048).  total_ms4 / launches4 point at 4 elements each.  Batches that
 * take another engine for a kind (small M) report 0 launches there. */
int rald_dit_profile_end_kinds(rald_dit* h, double* total_ms4, int32_t* launches4);
/* Between begin and end: which kinds are bracketed from now on (bit k = kind k; begin resets it to all four).  An event pair costs ~2.5 us of
 * stream time, 96 pairs per NFE at 24 blocks: a measurement that also reports the whole-job rate brackets the three residual + LayerNorm
 * kinds on a few NFEs only and the dominant kernel on all of them. */
int rald_dit_profile_set_kinds(rald_dit* h, uint32_t kind_mask);

/* ------------------------------------------------------------------------------------------
 * Set-latent autoencoder: KLAutoEncoder, query_type='mix' or 'learnable'  (model/models_ae.py:284-432)
 * ---------------------------------------------------------------------------------------- */
typedef struct rald_ae rald_ae;
typedef struct rald_ae_config {
    int32_t dim;          /* 512 (tiny config: 256)      create_autoencoder(dim=..) :434   */
    int32_t num_latents;  /* 512 (tiny: 128)             M                                  */
    int32_t latent_dim;   /* 32                          latent_dim                         */
    int32_t depth;        /* 24 (hard-coded :449)                                           */
    int32_t heads;        /* 8  (hard-coded :455)                                           */
    int32_t dim_head;     /* 64 (hard-coded :456)                                           */
    int32_t num_inputs;   /* P: encode asserts pc.shape[1] == num_inputs (:354)             */
    int32_t query_type;   /* 0 = 'mix' (:380-387, the shipped config), 1 = 'learnable' (:378-379: keys `latents.weight`
                             instead of s_latents / d_latents / mix_attn_layer / query_proj)   */
} rald_ae_config;

int rald_ae_create(const rald_ae_config* cfg, rald_ae** out);
void rald_ae_destroy(rald_ae* h);
int rald_ae_load_weight(rald_ae* h, const char* name, const float* data, int64_t nelem);
int rald_ae_finalize(rald_ae* h);
/* KLAutoEncoder.encode (:351-405): pc [B,P,3]; eps [B,M,latent_dim] = the posterior noise
 * (the reference draws it with torch.randn on the CPU global RNG, :153 - the caller passes it so
 * results are reproducible); outputs z [B,M,L], kl [B], and optionally mean / logvar [B,M,L]
 * (NULL to skip). */
int rald_ae_encode(rald_ae* h, const float* pc, int32_t batch, const float* eps, float* out_mean, float* out_logvar,
                   float* out_z, float* out_kl, void* stream);
/* decode (:408-424) split at its query-independent part: the latent stack (proj + depth x
 * [self-attention, GEGLU FF]) and the decoder context are computed ONCE per z into `ctx`
 * (rald_ae_ctx_bytes bytes, 16-byte aligned); any number of query sets can then be decoded
 * against it (the reference recomputes the 116-GFLOP stack for each of its <=4 decode calls per
 * sample, engine_generation.py:204, :275, :300). */
int64_t rald_ae_ctx_bytes(const rald_ae* h, int32_t batch);
int64_t rald_ae_workspace_generation(const rald_ae* h);   /* as rald_dit_workspace_generation */
int rald_ae_decode_latents(rald_ae* h, const float* z, int32_t batch, void* ctx, void* stream);
/* queries [B,Q,3] -> occupancy logits [B,Q] (the reference returns [B,Q,1]; occupied iff > 0) */
int rald_ae_decode_queries(rald_ae* h, const void* ctx, const float* queries, int32_t batch, int64_t n_queries,
                           float* out_logits, void* stream);
/* The same decoder on RAGGED query sets (the batched inference tail): queries [n_total,3] and out_logits [n_total] are the samples'
 * rows concatenated, offsets = DEVICE int64 [batch+1] with offsets[0] = 0 and sample b owning rows offsets[b] .. offsets[b+1]-1 (an
 * empty segment is legal, a segment may start anywhere); max_per_sample = a HOST upper bound of the longest segment (it sizes the
 * grid; nothing is read back, so the bound cannot be checked: with a bound BELOW the longest segment the rows behind it stay
 * unwritten and no error is returned).  A segment is cut into 64-query chunks from its own first row, so its logits are bit-identical
 * to rald_ae_decode_queries with the same ctx on that segment alone.  Rows from offsets[batch] on are not written. */
int rald_ae_decode_queries_ragged(rald_ae* h, const void* ctx, const float* queries, const int64_t* offsets, int32_t batch,
                                  int64_t max_per_sample, float* out_logits, void* stream);
/* Logit AND its gradient with respect to the query point, in the decoder's normalised coordinates (forward mode, closed form: DESIGN
 * section 18): out_logits [B,Q] are rald_ae_decode_queries' bit for bit, out_grad [B,Q,3].  out_projected (NULL to skip) [B,Q,3] is the
 * query after one clamped Newton step towards logit = 0: s = -logit g / |g|^2, scaled by min(1, max_step / |s|), s = 0 when |g|^2 is
 * not > 1e-20 or the step is not finite, then clamped to [-1,1] per axis; max_step must be finite and > 0 when out_projected is given.
 * num_latents <= 512 (a second, transposed image of the context shares LDS with the first); otherwise what the plain entries accept.
 * _ragged: layout, offsets and max_per_sample as rald_ae_decode_queries_ragged; all three outputs are bit-identical to the dense call
 * on the segment alone. */
int rald_ae_decode_queries_grad(rald_ae* h, const void* ctx, const float* queries, int32_t batch, int64_t n_queries, float* out_logits,
                                float* out_grad, float* out_projected, float max_step, void* stream);
int rald_ae_decode_queries_grad_ragged(rald_ae* h, const void* ctx, const float* queries, const int64_t* offsets, int32_t batch,
                                       int64_t max_per_sample, float* out_logits, float* out_grad, float* out_projected, float max_step,
                                       void* stream);
/* First-return beam casting through the decoder field (rald_amd/csrc/ae_rays.hip): a LiDAR-like scan of the sample
 * whose context is `ctx`, one launch.  origins / dirs fp32 in the decoder's normalised coordinates, ray r of the table is the segment
 * from o to o + d; ray_batch_stride (in floats) = 0 for one [n_rays,3] table shared by all samples, or 3 * n_rays for [batch,n_rays,3].
 * March: for k = 0 .. n_steps, t_k = (float)k / (float)n_steps, point o + t_k d (every operation rounded on its own); the ray hits at
 * the first k whose logit is > 0 (a NaN logit never hits): k_hit = k, hi = t_k, lo = t_(k-1) (k = 0: lo = hi = 0).  Refine: n_refine
 * bisection steps mid = 0.5f (lo + hi) for the rays with k_hit >= 1 (logit > 0: hi = mid; else lo = mid).  Every logit is
 * rald_ae_decode_queries' on the same [n_rays,3] points, bit for bit.  Outputs: out_t [batch,n_rays] = hi (-1: no return), out_logit
 * = the logit at hi (NaN: no return), out_step int32 = k_hit (-1), out_points (NULL to skip) [batch,n_rays,3] = o + hi d (NaN): always
 * a point at which the logit was seen > 0.  n_steps in [1,65535], n_refine in [0,30], n_rays in [1,2^28]; a refused call (bad counts,
 * another stride, a null required pointer) returns an error and leaves every output untouched. */
int rald_ae_cast_rays(rald_ae* h, const void* ctx, const float* origins, const float* dirs, int64_t ray_batch_stride, int32_t batch,
                      int64_t n_rays, int32_t n_steps, int32_t n_refine, float* out_t, float* out_logit, int32_t* out_step, float* out_points,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Radar-spectrum encoder alone: RadarAutoencoder.encoder / _encode (model/models_radar_encoder.py
 * :137-241, :390-393) - the frozen-encoder route of engine_generation.py:87, :191.  Keys are
 * those BELOW "encoder." in a RadarAutoencoder checkpoint.
 * ---------------------------------------------------------------------------------------- */
typedef struct rald_radar rald_radar;
int rald_radar_create(int32_t basic_channel, int32_t embed_dim, int32_t in_channels, int32_t R, int32_t A, int32_t E, rald_radar** out);
void rald_radar_destroy(rald_radar* h);
int rald_radar_load_weight(rald_radar* h, const char* name, const float* data, int64_t nelem);
int rald_radar_finalize(rald_radar* h);
/* cube [B,R,A,E,in_channels] -> z [B,R/16,A/16,E/16,embed_dim]  (= _encode's permuted output) */
int rald_radar_encode(rald_radar* h, const float* cube, int32_t batch, float* out_z, void* stream);
/* Decoder half (Decoder.forward :333-359, RadarAutoencoder.decode / forward :386-406): keys below "decoder." are loaded with
 * rald_radar_load_decoder_weight (optional: the generation path only encodes; once one is loaded rald_radar_finalize wants all).
 * z [B, R/16, A/16, E/16, embed_dim] (the layout rald_radar_encode returns) -> out_pred4 [B, R, A, E, 4] fp32: channels 0-1 are the
 * reconstruction (RadarAutoencoder.forward's 'pred' is out_pred4[..., :2]), channels 2-3 are zero padding of the convolution kernel. */
int rald_radar_load_decoder_weight(rald_radar* h, const char* name, const float* data, int64_t nelem);
int rald_radar_decode(rald_radar* h, const float* z, int32_t batch, float* out_pred4, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decode post-processing on the device (the host tail of engine_generation.evaluate, :229-243 and
 * :283-322; utils/utils.py:50-75 inverse_norm_points, :116-142 cal_metrics;
 * dataset_preprocessor/lidar.py:57-63 polar2cartesian)
 * ---------------------------------------------------------------------------------------- */
int64_t rald_post_scratch_bytes(int64_t n_queries);
/* np.where(logits > threshold) + grid[ind] + inverse_norm_points (+ polar2cartesian if view_cone_mode):
 * positives are written in ascending query index to out_points [<=Q,3] (out_index optional, may be
 * NULL), their number to *out_count (device int64).  pc_range6_host = [min0,min1,min2,max0,max1,max2] as DOUBLES
 * (the reference's ranges are Python floats; its isotropic branch adds a float64 offset). */
int rald_post_occupied_points(const float* logits, const float* queries, int64_t n_queries, const double* pc_range6_host,
                              int32_t norm_anisotropy, int32_t norm_isotropy, int32_t view_cone_mode, float threshold,
                              float* out_points, int64_t* out_index, int64_t* out_count, void* scratch, void* stream);
/* rald_post_occupied_points for a ragged batch (layout as rald_ae_decode_queries_ragged; in_offsets / out_offsets DEVICE int64
 * [batch+1]): the positives of every sample in ascending query order, the samples packed one behind the other in out_points
 * [<=n_total,3]; out_offsets[b] .. out_offsets[b+1]-1 are sample b's rows; out_index (optional) counts from the sample's first query.
 * Rows from in_offsets[batch] on (n_total may be a worst-case size) belong to no sample and are not counted.
 * scratch: rald_post_scratch_bytes(n_total), 8-byte aligned.  No host read. */
int rald_post_occupied_points_ragged(const float* logits, const float* queries, const int64_t* in_offsets, int32_t batch, int64_t n_total,
                                     const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy, int32_t view_cone_mode,
                                     float threshold, float* out_points, int64_t* out_index, int64_t* out_offsets, void* scratch, void* stream);
/* inverse_norm_points (+ polar2cartesian) of a whole array (the ground-truth surface, :290, :317) */
int rald_post_transform_points(const float* points, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy,
                               int32_t norm_isotropy, int32_t view_cone_mode, float* out_points, void* stream);
/* rald_post_transform_points (out_points: the same bits) + one unit normal per point: grad [n,3] is the logit's gradient in the
 * NORMALISED coordinates (rald_ae_decode_queries_grad); out_normals [n,3] = -J^-T grad / |J^-T grad| with J = d(metric point) /
 * d(normalised point), computed in double and rounded once: it points from occupied to empty.  (0,0,0) where the transform is singular
 * (range 0, the poles of the view cone), the gradient vanishes or anything is not finite.  _ragged: offsets DEVICE int64 [batch+1],
 * n_total may be a worst-case size; rows from offsets[batch] on are not written.  No host read. */
int rald_post_oriented_points(const float* points, const float* grad, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy,
                              int32_t norm_isotropy, int32_t view_cone_mode, float* out_points, float* out_normals, void* stream);
int rald_post_oriented_points_ragged(const float* points, const float* grad, const int64_t* offsets, int32_t batch, int64_t n_total,
                                     const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy, int32_t view_cone_mode,
                                     float* out_points, float* out_normals, void* stream);
/* cal_metrics' two sums (exact nearest neighbour, fp64): out_sums2[0] = sum_pred min_gt ||.||,
 * out_sums2[1] = sum_gt min_pred ||.||;  chamfer = 0.5*out[0]/n_pred + 0.5*out[1]/n_gt */
int rald_post_chamfer_sums(const float* pred, int64_t n_pred, const float* gt, int64_t n_gt, double* out_sums2, void* stream);
/* rald_post_chamfer_sums per sample of a ragged batch: out_sums [batch,2] (device doubles, zeroed here); max_pred / max_gt = HOST upper
 * bounds of the longest segment of either side (they size the grids; the device offsets are not read back, so a bound BELOW a segment's
 * length silently leaves that segment's rows behind the bound out of its sum).  A sample with an empty side keeps 0 for that sum. */
int rald_post_chamfer_sums_ragged(const float* pred, const int64_t* pred_offsets, const float* gt, const int64_t* gt_offsets, int32_t batch,
                                  int64_t max_pred, int64_t max_gt, double* out_sums, void* stream);
/* ---- point-cloud metrics: exact nearest neighbours in float64 (coordinates fp32 in; d^2 = dx*dx + dy*dy + dz*dz,
 * every operation rounded, left to right), ragged batches as above (DEVICE int64 offsets [batch+1], HOST upper bounds of the longest
 * segment of either side that size the grids and the scratch).  Nothing is read back, so the bounds cannot be checked: a bound BELOW a
 * segment's length silently gives PARTIAL results (the rows behind it get no output and enter no sum, the candidates behind it are not
 * searched) and no error.  No atomics: every result is the same bits in every call, for every chunk length and in every batch.
 * Scratch of the rald_post_* calls: rald_post_cloud_metrics_scratch_bytes of the same batch and bounds (for rald_post_nn_ragged with
 * max_pred = max_a, max_gt = max_b), 8-byte aligned; -1 for arguments the calls refuse. */
int64_t rald_post_cloud_metrics_scratch_bytes(int32_t batch, int64_t max_pred, int64_t max_gt);
/* per row of a: out_dist (double) = distance to the nearest row of b in the same sample, out_idx (int64) = that row's index from the
 * sample's first b row; equal distances: the lowest index.  Either output may be NULL.  Outputs are laid out like a (row a_offsets[s] + i);
 * rows from a_offsets[batch] on are not written.  A sample without b rows gets dist = inf, idx = -1. */
int rald_post_nn_ragged(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int32_t batch, int64_t max_a,
                        int64_t max_b, double* out_dist, int64_t* out_idx, void* scratch, void* stream);
/* both directions (0: pred -> gt, 1: gt -> pred) and their reductions: out_raw [batch,2,3+K] doubles = sum of d, sum of d^2, max of d,
 * number of rows with d < thresholds_host[k] (strict, in float64, on d) for the K = n_thresholds <= 8 HOST doubles (finite, >= 0).
 * The sums run in a fixed order counted from the sample's own first row: a sample's out_raw is the same bits alone and in any batch.
 * A sample with an empty side gets zeros.  The four per-row outputs (as rald_post_nn_ragged) may each be NULL. */
int rald_post_cloud_metrics_ragged(const float* pred, const int64_t* pred_offsets, const float* gt, const int64_t* gt_offsets, int32_t batch,
                                   int64_t max_pred, int64_t max_gt, const double* thresholds_host, int32_t n_thresholds, double* out_raw,
                                   double* out_dist_pred, int64_t* out_idx_pred, double* out_dist_gt, int64_t* out_idx_gt, void* scratch,
                                   void* stream);
/* rald_post_nn_ragged with an explicit chunk length (test-facing: several chunks at small sizes): the b rows one workgroup searches,
 * 0 = the automatic choice (a function of batch, max_a and max_b only), otherwise a multiple of 1024.  scratch_bytes >=
 * rald_op_nn_scratch_bytes of the same arguments. */
int64_t rald_op_nn_scratch_bytes(int32_t batch, int64_t max_a, int64_t max_b, int64_t b_chunk);
int rald_op_nn_ragged(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int32_t batch, int64_t max_a,
                      int64_t max_b, int64_t b_chunk, double* out_dist, int64_t* out_idx, void* scratch, int64_t scratch_bytes, void* stream);
/* ---- farthest-point sampling: k rows per cloud, each the row farthest from the rows chosen so far.  Defined
 * to the bit, so the result is the same in every call and in every batch:
 *   p' = fl(p * scale) per coordinate, once (scale3_host: 3 HOST floats, NULL = 1, 1, 1);
 *   d2(i, j) = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), dx = fl(p'_i.x - p'_j.x) ...: fp32, round to nearest, no contraction;
 *   mind[i] = +inf; the first choice is start[b] mod n (non-negative modulo; start: DEVICE int64 [batch], NULL = 0); after a choice c,
 *   mind[i] = min(mind[i], d2(i, c)); the next choice is the i of the largest mind[i], the SMALLEST such i on equal values.
 * Chosen rows are not excluded: once fewer than k distinct points remain, the smallest index repeats with distance 0.
 * out_idx int64 [batch,k]: row indices from the cloud's own first row; out_dist2 fp32 [batch,k] (may be NULL): +inf in slot 0, then
 * mind of the chosen row when it was chosen.  A cloud of n < k rows gets its n choices, then idx = -1 and dist2 = NaN; n = 0: all.
 * Layout: points [T,3]; offsets DEVICE int64 [batch+1], or NULL for dense clouds of n_dense rows each (cloud b at row b * n_dense);
 * counts DEVICE int32 [batch] or NULL: the valid rows from the cloud's first row (the cropped LiDAR layout), capped at the segment.
 * max_per_sample: HOST bound of the longest cloud, 1 .. 65536.  Nothing is read back, so it cannot be checked: a cloud LONGER than
 * the bound is sampled from its FIRST max_per_sample rows only, silently.
 * Coordinates must be finite.  With non-finite ones the choice is unspecified, but every index written lies in [0, n) and no address
 * depends on the data.  One workgroup per cloud; the loop runs min(k, n) - 1 times and waits on no other workgroup.
 * form: 0 = automatic (resident up to 16384, streaming above), 1 = resident (coordinates in registers, max_per_sample <= 16384),
 * 2 = streaming (coordinates re-read from a scaled copy in scratch); test-facing, the result does not depend on it.
 * scratch: rald_post_fps_scratch_bytes of the same batch, bound and form (0 bytes for the resident form: scratch may then be NULL),
 * 16-byte aligned; -1 (and rald_last_error) for arguments the call refuses. */
int64_t rald_post_fps_scratch_bytes(int32_t batch, int64_t max_per_sample, int32_t form);
int rald_post_fps_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                         int64_t max_per_sample, int32_t k, const int64_t* start, const float* scale3_host, int64_t* out_idx, float* out_dist2,
                         void* scratch, int64_t scratch_bytes, int32_t form, void* stream);
/* ---- voxel-grid down-sampling: every cloud of a ragged batch becomes one point per occupied cell of a fixed
 * grid.  Defined to the bit, so the result is the same in every call, in every batch and for every chunk length:
 *   grid (HOST values): lo3_host 3 floats (finite), v3_host 3 floats (the cell edge per axis, finite and > 0), dims3_host 3 int32
 *   (>= 1), cells = dims0 * dims1 * dims2 <= 2^31 - 1.
 *   cell of a row, per axis: c = floorf(fl(fl(p - lo) / v)): fp32, round to nearest, no contraction, the division correctly rounded.
 *   The row is inside iff 0 <= c < (float)dims on all three axes, compared in float before any conversion (NaN, +-inf: outside).
 *   key = (c0 * dims1 + c1) * dims2 + c2.  Rows outside are dropped: counted nowhere, out_inverse -1.
 *   voxels of a cloud: the distinct keys of its inside rows in ASCENDING KEY order (a canonical order, independent of the row order).
 *   out_points fp32 [n_total,3]: the centroid - per coordinate the voxel's rows added in float64 in ascending row order, left to
 *   right, divided by (double)n, rounded to fp32 once.  out_offsets DEVICE int64 [batch+1]: cloud b's voxels are rows
 *   out_offsets[b] .. out_offsets[b+1]-1, the clouds packed one behind the other; rows from out_offsets[batch] on are not written.
 *   Optional (NULL = not wanted), one per voxel: out_count int32 (rows in the voxel), out_first int64 (its smallest row index, from the
 *   cloud's first row), out_cells int32 [n_total,3] (c0, c1, c2).  Optional per row, laid out like points: out_inverse int64 [n_total],
 *   the rank of the row's voxel inside its cloud, -1 for a dropped row.
 * Layout: points [n_total,3]; offsets DEVICE int64 [batch+1], or NULL for dense clouds of n_dense rows each; counts DEVICE int32
 * [batch] or NULL: the valid rows from the cloud's first row, capped at the segment; rows behind counts[b] are neither read nor written.
 * max_per_sample: HOST bound of the longest cloud, 1 .. 16777216; it is trusted and sizes grids and scratch: a cloud LONGER than the
 * bound is reduced from its FIRST max_per_sample rows, silently (the rows behind get no out_inverse).  A cloud's span is clamped into
 * [0, n_total] on the device: no access leaves points, the outputs or the scratch whatever offsets and bound hold.  batch 1 .. 65535,
 * n_total 0 .. 2^31 - 1.
 * Separate launches, none waits on another workgroup; no float atomics.  The sort is a stable LSD radix sort of (key, row), 8 bits
 * per pass, rald_op_voxel_passes(cells) = ceil(bits(cells) / 8) passes; a cloud bound above one chunk is sorted by one workgroup per
 * chunk, one that fits a chunk by one workgroup per cloud.  One lane adds a voxel's rows: the time of a cloud with ALL rows in one
 * cell grows with its length.
 * scratch: rald_post_voxel_scratch_bytes of the same batch, n_total and bound, 16-byte aligned, never NULL; -1 (and rald_last_error)
 * for sizes the call refuses.  Every invalid argument is refused with a status before any GPU work.
 * rald_op_*: test-facing, with the chunk length of the split sort: 0 = automatic (what rald_post_* uses), else a multiple of 1024; a
 * chunk >= max_per_sample forces the one-workgroup sort.  The result does not depend on it. */
int64_t rald_post_voxel_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample);
int rald_post_voxel_downsample_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                      int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                      const int32_t* dims3_host, float* out_points, int64_t* out_offsets, int32_t* out_count, int64_t* out_first,
                                      int32_t* out_cells, int64_t* out_inverse, void* scratch, int64_t scratch_bytes, void* stream);
int64_t rald_op_voxel_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int32_t rald_op_voxel_passes(int64_t cells);
int rald_op_voxel_downsample_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                    int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                    const int32_t* dims3_host, float* out_points, int64_t* out_offsets, int32_t* out_count, int64_t* out_first,
                                    int32_t* out_cells, int64_t* out_inverse, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream);
/* ---- fixed-radius neighbours inside a cloud and the radius outlier filter.  Defined to the bit, so the result
 * is the same in every call, in every batch, for every chunk length and for every cell edge the call accepts:
 *   Layout and grid are those of rald_post_voxel_downsample_ragged: points fp32 [n_total,3]; offsets DEVICE int64 [batch+1], or NULL
 *   for dense clouds of n_dense rows; counts DEVICE int32 [batch] or NULL; max_per_sample a trusted HOST bound, 1 .. 16777216 (a
 *   LONGER cloud is treated as its FIRST max_per_sample rows, silently); a cloud's span is clamped into [0, n_total] on the device.
 *   lo3_host, v3_host, dims3_host as there, cells <= 2^31 - 1.  A row is INSIDE iff 0 <= c < (float)dims on all three axes, with
 *   c = floorf(fl(fl(p - lo) / v)) in fp32 without contraction.  Rows outside (NaN and +-inf included) take no part: they are
 *   nobody's neighbour, their own count is -1, their nearest is -1 / +inf, and the filter drops them.
 *   radius: a HOST float, finite and > 0, and v >= radius on every axis (else the call is refused); r2 = fl(radius * radius) in fp32.
 *   d2(i, j) = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), dx = fl(p_j.x - p_i.x) ...: fp32, round to nearest, no contraction.
 *   count[i] = the number of inside rows j != i of the same cloud with d2(i, j) <= r2.  j != i is by row index: a duplicate of row i
 *   counts.  With max_count = m > 0 the value is min(count, m) (the search of a row stops there); max_count = 0: no cap.
 *   Nearest other row (out_nn_idx, out_nn_dist2: each may be NULL; either one requires max_count = 0): out_nn_idx int64 = the j of the
 *   smallest d2 among the counted rows, the SMALLEST row index on equal d2, counted from the cloud's first row, -1 when count = 0;
 *   out_nn_dist2 fp32 = that d2, +inf when there is none.
 *   The three per-row outputs are laid out like points (row offsets[b] + i); rows outside every cloud's span are not written.
 *   Filter: row i is kept iff it is inside and count[i] >= min_neighbors (>= 1; 0 is refused).  Kept rows come out in their ORIGINAL
 *   row order, the clouds packed one behind the other as rald_post_occupied_points_ragged packs them: out_points fp32 [n_total,3] (the
 *   input row's bits), out_offsets DEVICE int64 [batch+1], optional out_index int64 [n_total] (the kept row's index from its cloud's
 *   first row), optional out_count int32 per INPUT row (min(count, min_neighbors), -1 outside).  Rows from out_offsets[batch] on are
 *   not written.
 * Every output is a function of the cloud's own rows, radius, lo3 and dims3 alone: v3 beyond v >= radius, the chunk, the batch and the
 * call do not show.  The grid is the index of the search, a stable radix sort of (cell key, row) - the one of the voxel call.  One
 * lane per sorted position scans, per axis, the cells cell(nextafterf(fl(p - rs), -inf)) .. cell(nextafterf(fl(p + rs), +inf)),
 * rs = fl(radius * (1 + 2^-20)), clamped to the grid, with the same cell function: fl(dx*dx) <= d2 <= r2 bounds the real offset per
 * axis by radius * (1 + 2^-22), the nextafter makes the bound hold at any magnitude, and the cell function is monotone, so no row
 * within r2 lies outside the scan; with v >= radius that is at most 4 cells per axis where a cell is wider than the coordinates' ulp.
 * No atomics, no kernel waits on another workgroup.  Without a cap a row's time grows with the rows around it: a cloud with ALL n
 * rows in one cell costs n * n distances; with a cap (the filter always has one) the walk stops at the cap.
 * scratch: rald_post_radius_scratch_bytes of the same batch, n_total and bound (one size serves both calls), 16-byte aligned, never
 * NULL; -1 (and rald_last_error) for sizes the calls refuse.  Every invalid argument is refused with a status before any GPU work.
 * rald_op_*: test-facing, with the chunk length of the split sort: 0 = automatic (what rald_post_* uses), else a multiple of 1024; a
 * chunk >= max_per_sample forces the one-workgroup sort.  The result does not depend on it. */
int64_t rald_post_radius_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample);
int rald_post_radius_count_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                  const int32_t* dims3_host, float radius, int32_t max_count, int32_t* out_count, int64_t* out_nn_idx,
                                  float* out_nn_dist2, void* scratch, int64_t scratch_bytes, void* stream);
int rald_post_radius_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                   int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                   const int32_t* dims3_host, float radius, int32_t min_neighbors, float* out_points, int64_t* out_offsets,
                                   int64_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, void* stream);
int64_t rald_op_radius_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int rald_op_radius_count_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                const int32_t* dims3_host, float radius, int32_t max_count, int32_t* out_count, int64_t* out_nn_idx,
                                float* out_nn_dist2, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream);
int rald_op_radius_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                 int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                 const int32_t* dims3_host, float radius, int32_t min_neighbors, float* out_points, int64_t* out_offsets,
                                 int64_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream);
/* ---- k nearest other rows inside a cloud and the statistical outlier filter.  Defined to the bit, so the
 * result is the same in every call, in every batch, for every chunk length and for every grid over the same box:
 *   Layout, grid, INSIDE and d2(i, j) are exactly those of rald_post_radius_count_ragged: points fp32 [n_total,3]; offsets DEVICE int64
 *   [batch+1], or NULL with n_dense; counts optional; max_per_sample a trusted HOST bound, 1 .. 16777216; lo3_host, v3_host, dims3_host
 *   with cells <= 2^31 - 1; d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) in fp32 without contraction; rows outside the box (NaN,
 *   +-inf) take no part.
 *   k: a HOST value, 1 .. 32.  max_radius: a HOST float, 0 = none, otherwise finite and > 0, r2max = fl(max_radius * max_radius).
 *   The CANDIDATES of an inside row i are the inside rows j != i of its cloud (by row index: a duplicate of row i is a candidate at
 *   distance 0), with max_radius only those with d2(i, j) <= r2max, ordered by the pair (d2(i, j), j) ascending - on equal distances
 *   the SMALLER row index comes first.
 *   Outputs per INPUT row, laid out like points: out_idx int64 [n_total,k], slot s = the s-th candidate's row index from the cloud's
 *   first row; out_dist2 fp32 [n_total,k] (may be NULL) its d2; out_found int32 [n_total] (may be NULL) = min(k, number of candidates),
 *   -1 for a row outside.  Slots from `found` on hold -1 / +inf; a row outside holds that in every slot.  Rows outside every cloud's
 *   span are not written.
 *   Every output is a function of the cloud's own rows, k, max_radius and the box (through which rows are inside) alone: the cell
 *   edge, the chunk, the batch and the call do not show, and no relation between v3 and max_radius is asked for.
 * Statistical outlier removal: k and max_radius as above; std_ratio a HOST double, finite and >= 0.
 *   m[i] (float64) = the sum over the slots s = 0 .. found-1, in that order, of sqrt((double)dist2[s]), divided by (double)found; the
 *   square root and the division correctly rounded.  found = 0: m = +inf.  A row outside: NaN.
 *   F = the inside rows of the cloud with found >= 1, n_f = |F|.  Cloud sums have ONE FIXED SHAPE, so that they depend on the cloud
 *   alone: the cloud's rows in row order, a row not in F as +0.0, padded with +0.0 to a multiple of 1024; inside block g (rows 1024g ..
 *   1024g+1023) for h = 512, 256, .., 1: v[t] += v[t+h] for t < h; the cloud's sum is s = 0.0; s += v_g[0] for g ascending.
 *   mu = SUM(m) / n_f; sigma = n_f >= 2 ? sqrt(SUM((m - mu) * (m - mu)) / (n_f - 1)) : 0; thr = fl(mu + fl(std_ratio * sigma)); all
 *   float64 without contraction.  Row i is KEPT iff it is in F and m[i] <= thr.  n_f = 0: nothing is kept, mu = sigma = thr = NaN.
 *   Outputs as the radius filter's: out_points (the kept rows in their order, the input row's bits), out_offsets DEVICE int64
 *   [batch+1], optional out_index int64 [n_total]; optional out_mean float64 [n_total] (m per INPUT row), optional out_stats float64
 *   [batch,3] = mu, sigma, thr.
 *   Where this differs from the usual libraries (Open3D remove_statistical_outlier, PCL StatisticalOutlierRemoval; neither is
 *   available to check against, so their conventions are stated from their documentation, unchecked): k counts OTHER rows, where
 *   Open3D's nb_neighbors includes the point itself; the filter keeps m <= thr, so a cloud of equal means is kept whole; the
 *   deviation divides by n_f - 1.
 * One lane per sorted position keeps its best-k list in LDS and scans a growing box of cells of the radius search's index; it stops
 * when the scanned box holds, on all three axes, the radius search's scan range for a float r with fl(r * r) >= w - w the list's worst
 * d2 once it holds k entries, else r2max - or the whole grid (DESIGN.md section 23 has the proof).  A row far from all others scans
 * the grid: its time grows with the grid's x extent and the rows of the cloud.  No atomics, no kernel waits on another workgroup.
 * The filter never holds the [n_total,k] tables: its scratch does not depend on k.
 * found = -2 cannot occur: it would say that the search ran out of its bound of 40 boxes (at most 35 are possible) before its list
 * was final, and such a row counts as outside.
 * n_total = 0 is accepted (nothing is written but out_offsets and out_stats), but points and the required outputs must still be
 * non-NULL pointers.
 * scratch: rald_post_knn_scratch_bytes / rald_post_statistical_scratch_bytes of the same batch, n_total and bound, 16-byte aligned,
 * never NULL; -1 (and rald_last_error) for sizes the calls refuse.  Every invalid argument is refused with a status before any GPU
 * work.  rald_op_*: test-facing, with the chunk length of the split sort as in the radius calls. */
int64_t rald_post_knn_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample);
int rald_post_knn_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense, int64_t n_total,
                         int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, int32_t k,
                         float max_radius, int64_t* out_idx, float* out_dist2, int32_t* out_found, void* scratch, int64_t scratch_bytes,
                         void* stream);
int64_t rald_post_statistical_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample);
int rald_post_statistical_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                        int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                        const int32_t* dims3_host, int32_t k, float max_radius, double std_ratio, float* out_points,
                                        int64_t* out_offsets, int64_t* out_index, double* out_mean, double* out_stats, void* scratch,
                                        int64_t scratch_bytes, void* stream);
int64_t rald_op_knn_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int rald_op_knn_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense, int64_t n_total,
                       int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, int32_t k,
                       float max_radius, int64_t* out_idx, float* out_dist2, int32_t* out_found, void* scratch, int64_t scratch_bytes,
                       int64_t chunk, void* stream);
int64_t rald_op_statistical_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int rald_op_statistical_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                      int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                      const int32_t* dims3_host, int32_t k, float max_radius, double std_ratio, float* out_points,
                                      int64_t* out_offsets, int64_t* out_index, double* out_mean, double* out_stats, void* scratch,
                                      int64_t scratch_bytes, int64_t chunk, void* stream);
/* ---- PCA normals, surface variation and covariance eigenvalues of every row from its k nearest other rows, and the normal consistency
 * of two ragged batches with normals.  Defined to the bit, so the result is the same in every call, in every
 * batch, for every chunk length and for every grid over the same box:
 *   Layout, grid, INSIDE, k (1 .. 32), max_radius (0 = none) and the candidates in their order (d2, j) are exactly those of
 *   rald_post_knn_ragged; `found` is its out_found.
 *   The NEIGHBOURHOOD of an inside row i with found >= 2 is row i first, then its found neighbours in slot order: m = found + 1 points.
 *   All arithmetic below is float64 on the fp32 coordinates, one rounded operation at a time, no contraction; every sum starts from
 *   +0.0 and adds its terms in the order given.
 *   mean c = (sum of the points in that order) / m, per coordinate.
 *   moments xx, xy, xz, yy, yz, zz: with d = p - c per coordinate, the sum over the points in that order of dx*dx, dx*dy, dx*dz, dy*dy,
 *   dy*dz, dz*dz, each divided by m.  A = the symmetric matrix of them (axes 0, 1, 2), V = the identity.
 *   Eigen-decomposition: SIX sweeps, each the pairs (p, q) = (0, 1), (0, 2), (1, 2) in that order, r the third axis.  A pair whose
 *   a_pq is exactly 0 is skipped; otherwise
 *     theta = (a_qq - a_pp) / (2 * a_pq);  t = sgn / (|theta| + sqrt(theta * theta + 1)), sgn = -1 for theta < 0, else +1;
 *     c = 1 / sqrt(t * t + 1);  s = t * c;  h = t * a_pq;
 *     a_pp = a_pp - h;  a_qq = a_qq + h;  a_pq = 0;
 *     (a_rp, a_rq) = (c * a_rp - s * a_rq, s * a_rp + c * a_rq);
 *     for every row u = 0, 1, 2 of V: (v_up, v_uq) = (c * v_up - s * v_uq, s * v_up + c * v_uq).
 *   There is no data-dependent stop.  (An overflowing theta gives t = 0: no rotation.)
 *   The eigenvalues are the diagonal, column u of V the vector of a_uu.  They are ordered ascending by three exchanges of neighbours -
 *   (0, 1), (1, 2), (0, 1), an exchange iff the first is GREATER - so equal eigenvalues keep the lower column first.  l0 <= l1 <= l2.
 *   out_eigenvalues fp32 [n_total,3] (may be NULL): l0, l1, l2 rounded to fp32.
 *   out_curvature fp32 [n_total] (may be NULL): the surface variation l0 / ((l0 + l1) + l2), 0 where that sum is 0.
 *   out_normals fp32 [n_total,3]: n = the column of l0, every component divided by sqrt((x*x + y*y) + z*z), then the sign, then fp32.
 *   Sign: with view3_host (3 HOST floats, finite; may be NULL) s = (n0 * (view0 - p0) + n1 * (view1 - p1)) + n2 * (view2 - p2), view
 *   and the row p converted to float64 first; n is negated iff s < 0.  Without a view, or with s == 0: the component of the largest
 *   magnitude (the lowest axis on equal magnitudes) is made positive.
 *   UNDEFINED rows - outside the box, found < 2, found = -2 - get the normal (0, 0, 0) and NaN for curvature and eigenvalues.
 *   out_found int32 [n_total] (may be NULL) = the search's found.  Rows outside every cloud's span are not written.
 *   Where this differs from the usual libraries (Open3D estimate_normals with KDTreeSearchParamKNN and
 *   orient_normals_towards_camera_location, PCL NormalEstimation; stated from their documentation, UNCHECKED): k counts OTHER rows
 *   here, and the row itself is always part of its neighbourhood, so k = 15 here is knn = 16 there; PCL's curvature is the same
 *   surface variation; neither defines its eigen-solver, so their normals agree with these only to rounding, and in sign only where
 *   s is not 0.
 * The search is rald_post_knn_ragged's, one lane per sorted position; the lane then walks its own list and leaves the six moments and
 * found per row in the scratch: no [n_total,k] table exists, and the scratch does not depend on k.
 * Normal consistency of two ragged batches A = pred and B = gt with normals (layout of rald_post_nn_ragged: DEVICE int64 offsets
 * [batch+1], HOST bounds max_pred / max_gt of the longest segment, trusted as there; n_pred_total / n_gt_total: the rows of the
 * tensors of either side, which size the scratch, 0 .. 2^31 - 1 - a frame's span is clamped into them):
 *   for every row a of A: nn(a) = its exact nearest row of B in the same frame (rald_post_nn_ragged's, the lowest index on equal
 *   distances); term = |(n_a.x * n_nn.x + n_a.y * n_nn.y) + n_a.z * n_nn.z| in float64 on the fp32 normals.  The row COUNTS iff
 *   both normals are finite and not (0, 0, 0) and the frame has B rows.
 *   nc(A->B) = the sum of the terms of the counting rows in the fixed sum shape of the statistical filter (the frame's rows in row
 *   order, a row that does not count as +0.0, blocks of 1024, the halving tree, the blocks left to right) divided by their number;
 *   NaN for none.
 *   out_nc float64 [batch,3] = nc(pred->gt), nc(gt->pred), (nc(pred->gt) + nc(gt->pred)) / 2; out_counts int64 [batch,2] = the
 *   counting rows of either direction.
 * No atomics, one stream, no kernel waits on another workgroup.  n_total = 0 (and a total of 0) is accepted with non-NULL pointers.
 * scratch: the *_scratch_bytes of the same sizes, 16-byte aligned, never NULL; -1 (and rald_last_error) for sizes the calls refuse.
 * Every invalid argument is refused with a status before any GPU work.  rald_op_*: test-facing, with the chunk length of the split
 * sort as in the radius calls. */
int64_t rald_post_normals_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample);
int rald_post_normals_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                             int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host,
                             int32_t k, float max_radius, const float* view3_host, float* out_normals, float* out_curvature,
                             float* out_eigenvalues, int32_t* out_found, void* scratch, int64_t scratch_bytes, void* stream);
int64_t rald_op_normals_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int rald_op_normals_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense, int64_t n_total,
                           int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, int32_t k,
                           float max_radius, const float* view3_host, float* out_normals, float* out_curvature, float* out_eigenvalues,
                           int32_t* out_found, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream);
int64_t rald_post_normal_consistency_scratch_bytes(int32_t batch, int64_t n_pred_total, int64_t n_gt_total, int64_t max_pred, int64_t max_gt);
int rald_post_normal_consistency_ragged(const float* pred, const float* pred_normals, const int64_t* pred_offsets, int64_t n_pred_total,
                                        const float* gt, const float* gt_normals, const int64_t* gt_offsets, int64_t n_gt_total, int32_t batch,
                                        int64_t max_pred, int64_t max_gt, double* out_nc, int64_t* out_counts, void* scratch,
                                        int64_t scratch_bytes, void* stream);
/* ---- density clustering (DBSCAN) inside a cloud and the removal of small clusters.  Defined to the bit, so
 * the result is the same in every call, in every batch, for every chunk length and for every grid the call accepts:
 *   Layout, grid, INSIDE, d2(i, j) and r2 = fl(eps * eps) are exactly those of rald_post_radius_count_ragged (eps in radius' place: a
 *   HOST float, finite and > 0, v >= eps on every axis); min_points a HOST value >= 0.
 *   count[i] = the number of OTHER inside rows j of the same cloud with d2(i, j) <= r2, capped at min_points (-1 outside the box).
 *   CORE: an inside row with count[i] >= min_points.  min_points counts OTHER rows: Open3D's min_points = m is m - 1 here.  With
 *   min_points = 0 every inside row is core (Euclidean cluster extraction) and count is 0 for every inside row.
 *   CLUSTER: a connected component of the graph on the core rows with an edge where d2(i, j) <= r2 (d2 is symmetric in fp32:
 *   fl(a - b) = -fl(b - a)).  Its representative is its smallest row index; a cloud's clusters are numbered 0 .. C - 1 in ascending
 *   order of representative.
 *   BORDER: an inside row that is not core with a core row within r2.  It takes the cluster of the core row of the smallest d2, the
 *   smallest row index on equal d2 - a rule of the rows alone, where textbook DBSCAN depends on the order of the visit.
 *   out_labels int32 [n_total], laid out like points: the cluster for core and border rows, -1 for noise (inside, neither), -2 for a
 *   row outside the box (NaN and +-inf rows included; such rows are nobody's neighbour).  Rows outside every cloud's span (past
 *   offsets[batch], behind counts or the bound) are not written.
 *   out_num_clusters int32 [batch] = C.  out_sizes (nullable) int32 [n_total]: cloud b's cluster c at row offsets[b] + c = its core
 *   AND border rows, 0 at c >= C inside the span, not written outside the spans.  out_count (nullable) int32 [n_total] per row.
 *   Filter: row i is kept iff label[i] >= 0 and sizes[label[i]] >= min_cluster_size (>= 1); with largest_only != 0 the label must
 *   also be the cluster of the largest size, the smallest id on equal sizes.  Kept rows come out as the radius filter's: out_points
 *   (original order, the input row's bits), out_offsets DEVICE int64 [batch+1], optional out_index int64 [n_total]; out_labels int32
 *   [n_total] per KEPT row = its ORIGINAL cluster id (not renumbered), out_num_clusters int32 [batch] = C before the filter.  Rows
 *   from out_offsets[batch] on are not written.
 * Launches behind the index: the capped count (skipped for min_points = 0), a second walk that joins every core row with its core
 * neighbours of smaller row index in a concurrent union-find and notes a border row's nearest core row, a flatten, the block scans
 * of the compaction over the flags "core root" (the rank of a root is its cluster id), the labels and sizes, and for the filter an
 * argmax per cloud, the keep flags, the compaction and a gather of the kept rows' labels.  The union-find hooks the LARGER root under
 * the smaller with a device-scope compare-and-swap, so parent[x] <= x always, a component's final root is its smallest row, and no
 * result depends on the order in which workgroups arrive; inside that kernel every read of a parent is a device-scope atomic load.
 * Integer atomics only (compare-and-swap and min on the parents, add on the sizes); every loop is bounded by the cloud's length.
 * scratch: rald_post_cluster_scratch_bytes of the same batch, n_total and bound (one size serves both calls), 16-byte aligned, never
 * NULL; -1 (and rald_last_error) for sizes the calls refuse.  Every invalid argument is refused with a status before any GPU work,
 * eps before the grid.  rald_op_*: test-facing, with the chunk length of the split sort as in the radius calls. */
int64_t rald_post_cluster_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample);
int rald_post_cluster_labels_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                    int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                    const int32_t* dims3_host, float eps, int32_t min_points, int32_t* out_labels, int32_t* out_num_clusters,
                                    int32_t* out_sizes, int32_t* out_count, void* scratch, int64_t scratch_bytes, void* stream);
int rald_post_cluster_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                    int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                    const int32_t* dims3_host, float eps, int32_t min_points, int32_t min_cluster_size, int32_t largest_only,
                                    float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, int32_t* out_num_clusters,
                                    void* scratch, int64_t scratch_bytes, void* stream);
int64_t rald_op_cluster_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk);
int rald_op_cluster_labels_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                  const int32_t* dims3_host, float eps, int32_t min_points, int32_t* out_labels, int32_t* out_num_clusters,
                                  int32_t* out_sizes, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream);
int rald_op_cluster_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                  const int32_t* dims3_host, float eps, int32_t min_points, int32_t min_cluster_size, int32_t largest_only,
                                  float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, int32_t* out_num_clusters,
                                  void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream);
/* ---- RANSAC plane segmentation inside a cloud and the removal (or extraction) of its planes.  Defined to the
 * bit: the result is a function of (rows, parameters, seed) alone, the same in every call and at every batch position.
 *   Layout: points / offsets / counts / n_dense / n_total / max_per_sample are those of the other ragged calls.  There is no grid.
 *   USABLE: a row whose three coordinates are finite.
 *   HOST parameters: threshold t finite and > 0; num_hypotheses H in 1 .. 65536; max_planes K in 1 .. 8; min_inliers >= 3; refine 0 or
 *   1; seed int64; view3_host NULL (= 0, 0, 0) or three finite floats.
 *   ROUNDS: for round j = 0 .. K - 1, LIVE_j is the list of the cloud's usable rows that no earlier round labelled, in row order, m its
 *   length.  m < 3: the cloud is finished.
 *   HYPOTHESIS h of round j: philox4x32_10(counter = (h, j, 0, 0), key = (seed mod 2^32, 2)) -> words w0 .. w3 (key tags 0 and 1 are the
 *   sampler's; the cloud's index is NOT in the counter).  Rows i_k = LIVE_j[(w_k * m) >> 32], k = 0, 1, 2 (a 64-bit integer product) with
 *   coordinates p0, p1, p2.  All in fp32, every operation rounded once, no contraction: e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2 (each
 *   component fl(fl(a * b) - fl(c * d)): nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z, nz = e1x e2y - e1y e2x), len2 = fl(fl(fl(nx *
 *   nx) + fl(ny * ny)) + fl(nz * nz)).  INVALID if two of the three positions in LIVE_j coincide or len2 is not finite or not > 0.
 *   INLIER: a row p of LIVE_j with fl(s * s) <= fl(fl(t * t) * len2), s = fl(fl(fl(nx * dx) + fl(ny * dy)) + fl(nz * dz)), d = p - p0
 *   per component.  No square root, no division.  score[h] = the number of inliers, -1 for an invalid hypothesis.
 *   BEST: the largest score, the smallest h on equal scores.  No valid hypothesis or a best score below min_inliers: finished.
 *   PLANE, refine = 0: in float64, (x, y, z) = n / sqrt((nx nx + ny ny) + nz nz) from the fp32 n, c0 = p0.
 *   PLANE, refine = 1: over LIVE_j, a row that is no inlier of the best hypothesis contributing +0.0, in the FIXED SUM SHAPE - blocks of
 *   1024 consecutive positions of LIVE_j, inside a block the halving tree v[i] += v[i + h] for h = 512, 256 .. 1 over the 1024 values (the
 *   padding is +0.0), the blocks' sums added left to right from +0.0 - the float64 sums of x, y, z, divided by the inlier count: the
 *   centroid c; then in the same shape the six sums of (p - c)(p - c)^T (xx, xy, xz, yy, yz, zz), divided by the count; six cyclic
 *   Jacobi sweeps, the three exchanges and the renormalisation exactly as rald_post_normals_ragged's: (x, y, z) is the column of the
 *   smallest eigenvalue divided by its length, c0 = c.  Round j's inliers are then the rows of LIVE_j with
 *   |fl64(fl64(x * (px - c0x) + y * (py - c0y)) + z * (pz - c0z))| <= (double)t, x y z after the sign rule; fewer than min_inliers of
 *   them: the cloud is finished and plane j is not written.
 *   SIGN: sgn = (x * (vx - c0x) + y * (vy - c0y)) + z * (vz - c0z) in float64; (x, y, z) is negated iff sgn < 0, or sgn == 0 and the
 *   first non-zero of (x, y, z) is negative.  The plane is (a, b, c, d) = (x, y, z, -((x * c0x + y * c0y) + z * c0z)).
 *   out_planes double [batch, K, 4]: NaN for planes not found.  out_num_planes int32 [batch].  out_inliers (nullable) int32 [batch, K]:
 *   0 for planes not found.  out_best (nullable) int32 [batch, K]: the winning h of a plane that was written, -1 else.
 *   out_labels int32 [n_total], laid out like points: the round that took the row, -1 for a usable row that no plane took, -2 for an
 *   unusable row.  Rows outside every cloud's span (past offsets[batch], behind counts or the bound) are not written.
 *   Filter: keep_planes != 0 keeps the rows with label >= 0, keep_planes = 0 those with label -1 (ground removal at K = 1); unusable
 *   rows are never kept.  Kept rows come out as the radius filter's: out_points (original order, the input row's bits), out_offsets
 *   DEVICE int64 [batch+1], optional out_index int64 [n_total]; out_labels int32 [n_total] per KEPT row, out_planes and out_num_planes
 *   as above.  Rows from out_offsets[batch] on are not written.
 * Launches (cloud_plane.hip): an init, then per round the row-order compaction of the live rows, one lane per hypothesis (Philox, the
 * three rows, eight floats), the scoring kernel rows x hypotheses (a tile of 1024 live rows per workgroup in registers, the hypotheses
 * uniform per wave; ballot and popcount per wave, LDS per workgroup, one integer atomicAdd per workgroup and hypothesis), an argmax per
 * cloud, the inlier flags and block sums, one lane per cloud for the sums, the sweeps and the plane, the float64 flags, and the
 * labels.  The K rounds are a host loop with no host read; a finished cloud's later rounds do nothing.  Integer atomics only; every
 * loop is bounded by H, K, the cloud's length or 64; every index read from the scratch is clamped before it addresses anything.
 * scratch: rald_post_plane_scratch_bytes of the same batch, n_total, bound, H and K (one size serves both calls), 16-byte aligned,
 * never NULL; -1 (and rald_last_error) for sizes the calls refuse.  Every invalid argument is refused with a status before any GPU
 * work. */
int64_t rald_post_plane_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int32_t num_hypotheses, int32_t max_planes);
int rald_post_plane_segment_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                   int64_t n_total, int64_t max_per_sample, float threshold, int32_t num_hypotheses, int32_t max_planes,
                                   int32_t min_inliers, int32_t refine, int64_t seed, const float* view3_host, int32_t* out_labels,
                                   double* out_planes, int32_t* out_num_planes, int32_t* out_inliers, int32_t* out_best, void* scratch,
                                   int64_t scratch_bytes, void* stream);
int rald_post_plane_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, float threshold, int32_t num_hypotheses, int32_t max_planes,
                                  int32_t min_inliers, int32_t refine, int64_t seed, const float* view3_host, int32_t keep_planes,
                                  float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, double* out_planes,
                                  int32_t* out_num_planes, void* scratch, int64_t scratch_bytes, void* stream);
/* ---- ICP registration of ragged clouds, point-to-point and point-to-plane, and the rigid transform of a ragged batch (DESIGN.md
 * section 27).  Defined to the bit: the result is a function of (rows, normals, arguments) alone, the same in every call, at every batch
 * position, for every chunk length and for every grid the call accepts over the same box.
 *   PAIR b: the source cloud S_b (source / src_offsets / src_counts / src_n_dense / n_src_total / max_src: the layout of the other
 *   ragged calls) and the target cloud T_b (the same with its own arrays) of the same batch position; mode 1: target_normals fp32
 *   [n_tgt_total, 3], laid out like target (mode 0: ignored, may be NULL); init DEVICE float64 [batch, 12] = R row-major then t, NULL =
 *   the identity.
 *   HOST parameters: mode 0 = point, 1 = plane; max_distance finite and > 0; max_iterations 1 .. 64; tolerance a double >= 0;
 *   min_correspondences >= 1; the grid lo3 / v3 / dims3 as in the radius calls, every cell edge >= max_distance.
 *   The TARGET is indexed on the grid; a target row outside it (INSIDE is the radius calls' rule; NaN and +-inf rows are outside) is
 *   nobody's candidate.  The grid does not show otherwise.
 *   All float64 arithmetic below is one rounded operation at a time, no contraction, only + - * / and the correctly rounded square
 *   root; brackets give the order.  For iteration i = 0 .. max_iterations - 1 of a pair that is not finished, with its (R, t):
 *   1 MOVE.  A source row p is USABLE iff its three coordinates are finite.  p'_k = ((R_k0 px + R_k1 py) + R_k2 pz) + t_k, the
 *     coordinates converted to float64 first; pf = fp32(p').
 *   2 CORRESPOND.  q(p) = the inside target row of the smallest d2 = rad_d2(pf, q) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), dx =
 *     fl(q.x - pf.x), all fp32, among those with d2 <= fl(max_distance * max_distance); the LOWEST target row index (from the cloud's
 *     first target row) on equal d2.  The scan range around pf is the radius calls' (scan_reach); it holds every such row.  The row
 *     COUNTS iff it is usable, pf is finite (so p' did not overflow), q exists, and in mode 1 q's normal is finite and not (0, 0, 0).
 *   3 ACCUMULATE.  q and n in float64, d = p' - q per coordinate.  One EQUATION (n): c = p' x n with c0 = fl(p'1 n2) - fl(p'2 n1), c1 =
 *     fl(p'2 n0) - fl(p'0 n2), c2 = fl(p'0 n1) - fl(p'1 n0); J = (c0, c1, c2, n0, n1, n2); r = (n0 d0 + n1 d1) + n2 d2.  Its 28 PRODUCTS:
 *     J_i J_j for i <= j (i ascending, j ascending inside i: 21), J_i r (6), r r.  Mode 1: the row's contribution is the products of
 *     the equation of q's normal.  Mode 0: three equations, n = (1,0,0), (0,1,0), (0,0,1), computed by the same formulas (the
 *     multiplications by 0 and 1 included); the contribution is (products(e0) + products(e1)) + products(e2) entry by entry.  The
 *     29th entry is (d0 d0 + d1 d1) + d2 d2, once per row.  A row that does not count contributes +0.0 to every entry.
 *     The 29 sums over the cloud's SOURCE rows in row order have the FIXED SUM SHAPE of the statistical filter: blocks of 1024 rows
 *     from the cloud's first row, padded with +0.0, inside a block v[t] += v[t + h] for t < h, h = 512 .. 1, the blocks added left to
 *     right from +0.0.  count = the counting rows.
 *   4 SOLVE.  count < min_correspondences: FINISHED with status 2, (R, t) unchanged.  Else A = the symmetric 6 x 6 of the 21 sums, g
 *     the 6.  Cholesky A = L L^T column by column, j = 0 .. 5: s = A_jj; s = s - L_jk L_jk for k = 0 .. j - 1.  The pivot is ACCEPTED
 *     iff s is finite and s > A_jj * 2^-30; L_jj = sqrt(s); for i = j + 1 .. 5: t = A_ji; t = t - L_ik L_jk for k = 0 .. j - 1; L_ij =
 *     t / L_jj.  Forward, i = 0 .. 5: s = -g_i; s = s - L_ik y_k for k = 0 .. i - 1; y_i = s / L_ii.  Back, i = 5 .. 0: s = y_i; s =
 *     s - L_ki x_k for k = i + 1 .. 5; x_i = s / L_ii.  A refused pivot or an x_k that is not finite: FINISHED with status 3, (R, t)
 *     unchanged.  (The floor 2^-30 A_jj stands between the rounding noise of s, about 2^-50 A_jj, and a column within 3e-5 rad of
 *     the span of the earlier ones, which no registration can use: an exactly planar target in mode 1 is refused by rule.)
 *   5 UPDATE.  x = (w, u), a = w * 0.5, aa = (a0 a0 + a1 a1) + a2 a2, den = 1 + aa, c = 1 - aa.  The Cayley rotation, every entry one
 *     product, one sum, one division: dR = [ (c + w0 a0) / den, (w0 a1 - w2) / den, (w0 a2 + w1) / den ; (w1 a0 + w2) / den, (c + w1
 *     a1) / den, (w1 a2 - w0) / den ; (w2 a0 - w1) / den, (w2 a1 + w0) / den, (c + w2 a2) / den ] - a rotation for every a, no sine,
 *     no cosine.  R_ij <- (dR_i0 R_0j + dR_i1 R_1j) + dR_i2 R_2j; t_i <- ((dR_i0 t0 + dR_i1 t1) + dR_i2 t2) + u_i, both from the old
 *     R and t.
 *   6 FINISH.  step = max_k |x_k|; step <= tolerance, tested AFTER the update is applied: FINISHED with status 1.  A pair that ran
 *     all iterations has status 0.  `iterations` = the number of updates applied (so 0 for a pair that finished with status 2 or 3
 *     at iteration 0).
 *   7 EVALUATE.  After the loop, for every pair, steps 1 - 3 once more with the final (R, t): fitness = count / usable source rows (0
 *     for none), inlier_rmse = sqrt(SUM((d0 d0 + d1 d1) + d2 d2) / count) (0 for count 0).
 *   out_transform float64 [batch, 16]: row-major 4 x 4, rows (R_k0, R_k1, R_k2, t_k), the last 0 0 0 1.  out_stats float64 [batch, 4] =
 *   fitness, inlier_rmse, the last step (0 if no update was applied), the evaluation's sum of r r.  out_info int32 [batch, 3] = status,
 *   iterations, the evaluation's count.  out_corr (nullable) int64 [n_src_total] per source row: q's index from the cloud's first
 *   target row in the evaluation, -1 for none (q's normal does not show here).  out_moved (nullable) fp32 [n_src_total, 3]: pf of the final transform.  Rows outside every span are
 *   not written.  An empty source or target: the initial transform, status 2, iterations 0, zeros.
 *   Where this differs from Open3D registration_icp (stated from its documentation, UNCHECKED; it is not available to check against):
 *   its point-to-point step is the closed-form SVD fit, this one is a Gauss-Newton step of the same objective, so the fixed points
 *   agree and the paths do not; it stops on relative changes of fitness and RMSE, this one on the size of the update; its
 *   correspondence has no tie rule.  Rigid motion only: no scale, no robust kernel, no multi-scale schedule, no global initialisation.
 * Launches (cloud_icp.hip): the target's index once, and the same index build over the source under the initial transform, which only
 * orders the lanes of the search (rows of one cell share a wave; no result depends on it); per iteration one lane per source row (the
 * move and the radius walk over the target's index), one workgroup per 1024 source rows (the 29 block sums) and one wave per pair (a
 * lane per sum for the blocks, then the solve, the update, the status); the same three once more for the evaluation.  The iterations are a host loop with no host read; a finished pair's later kernels
 * return at once.  One stream, no kernel waits on another workgroup, no atomics; every loop is bounded by a cloud's length, the scan
 * range or a constant; every index read from the scratch is clamped before it addresses anything.
 * scratch: rald_post_icp_scratch_bytes of the same sizes, 16-byte aligned, never NULL; -1 (and rald_last_error) for sizes the calls
 * refuse.  Every invalid argument is refused with a status before any GPU work.  rald_op_*: test-facing, with the chunk length of the
 * target's split sort as in the radius calls.
 * Rigid transform of a ragged batch: transforms DEVICE float64 [batch, transform_stride], transform_stride 12 (R row-major, then t) or
 * 16 (row-major 4 x 4, the last row ignored).  out_points fp32 [n_total, 3] = step 1's pf of every row of a span (non-finite rows
 * included: they come out as the arithmetic gives them); with normals fp32 [n_total, 3] (nullable, with out_normals) out_normals =
 * step 1's pf of the normal with t = +0.0: the rotation alone.  In place (out_points == points) is allowed. */
int64_t rald_post_icp_scratch_bytes(int32_t batch, int64_t n_src_total, int64_t max_src, int64_t n_tgt_total, int64_t max_tgt);
int rald_post_icp_ragged(const float* source, const int64_t* src_offsets, const int32_t* src_counts, int64_t src_n_dense, int64_t n_src_total,
                         int64_t max_src, const float* target, const int64_t* tgt_offsets, const int32_t* tgt_counts, int64_t tgt_n_dense,
                         int64_t n_tgt_total, int64_t max_tgt, const float* target_normals, int32_t batch, const float* lo3_host,
                         const float* v3_host, const int32_t* dims3_host, int32_t mode, float max_distance, int32_t max_iterations,
                         double tolerance, int32_t min_correspondences, const double* init, double* out_transform, double* out_stats,
                         int32_t* out_info, int64_t* out_corr, float* out_moved, void* scratch, int64_t scratch_bytes, void* stream);
int64_t rald_op_icp_scratch_bytes(int32_t batch, int64_t n_src_total, int64_t max_src, int64_t n_tgt_total, int64_t max_tgt, int64_t chunk);
int rald_op_icp_ragged(const float* source, const int64_t* src_offsets, const int32_t* src_counts, int64_t src_n_dense, int64_t n_src_total,
                       int64_t max_src, const float* target, const int64_t* tgt_offsets, const int32_t* tgt_counts, int64_t tgt_n_dense,
                       int64_t n_tgt_total, int64_t max_tgt, const float* target_normals, int32_t batch, const float* lo3_host,
                       const float* v3_host, const int32_t* dims3_host, int32_t mode, float max_distance, int32_t max_iterations,
                       double tolerance, int32_t min_correspondences, const double* init, double* out_transform, double* out_stats,
                       int32_t* out_info, int64_t* out_corr, float* out_moved, void* scratch, int64_t scratch_bytes, int64_t chunk,
                       void* stream);
int rald_post_rigid_transform_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                     int64_t n_total, int64_t max_per_sample, const double* transforms, int32_t transform_stride,
                                     const float* normals, float* out_points, float* out_normals, void* stream);
/* ---- Isosurface meshing of a batch of dense volumes by naive surface nets: one vertex per sign-changing cell,
 * one quad per sign-changing grid edge.  Defined to the bit: the result is a function of (values, iso, lo, spacing, dims) alone, the
 * same in every call and at every batch position.
 *   volume fp32 [batch, nx, ny, nz], z fastest.  Node (i, j, k) sits at fl(lo_a + fl((float)i_a * h_a)) per axis a (rald_query_grid
 *   gives these positions).  HOST parameters: lo3 finite, spacing3 = h finite and > 0, dims3 = (nx, ny, nz) each 2 .. 1024, iso not a
 *   NaN, batch 1 .. 65535 and batch * nx * ny * nz <= 357913941 = (2^31 - 1) / 6 (six triangles a node at most, counted in int32: a batch
 *   of 8 volumes of 256^3 passes, one volume of 1024^3 does not).
 *   INSIDE: a node is inside iff value > iso, the comparison of rald_post_occupied_points; a NaN is outside.
 *   CELL (i, j, k), 0 <= i_a < n_a - 1, linear index (i * (ny - 1) + j) * (nz - 1) + k, ACTIVE iff its 8 corners are not all on one
 *   side.  Its 12 edges: e = 4 * axis + 2 * p + q, p and q the 0 / 1 offsets along the two other axes in ascending axis order.  Edge e
 *   CROSSES iff its two end nodes differ in INSIDE.
 *   VERTEX of an active cell, all fp32, one rounded operation at a time, no contraction: for every crossing edge in ascending e, t =
 *   fl(fl(iso - a) / fl(b - a)), a the value at the edge's lower node and b at its upper; a NaN t becomes 0; then t < 0 becomes 0 and
 *   t > 1 becomes 1.  The edge's point in cell units is t on the edge's axis and (float)p, (float)q on the others.  u = the
 *   per-component sum of these points, from +0.0 and in that order, divided by (float)count.  The vertex is fl(lo_a + fl(fl((float)i_a
 *   + u_a) * h_a)).  Volume b's vertices are its active cells in ascending linear index, numbered from 0 inside the volume.
 *   FACE: a grid edge along axis a from node n to n + e_a that crosses, (u, w) the other two axes in cyclic order (y, z), (z, x), (x,
 *   y), makes a face only if n_u and n_w both lie in 1 .. dims - 2 (the four cells around the edge exist).  The cells by their (u, w)
 *   offsets from n, the offset on axis a zero: c0 = (-1, -1), c1 = (0, -1), c2 = (0, 0), c3 = (-1, 0).  n inside: triangles (c0, c1,
 *   c2), (c0, c2, c3); else (c0, c2, c1), (c0, c3, c2): counter-clockwise seen from the empty side.  Faces in ascending ((i * ny + j) *
 *   nz + k) * 3 + a of (n, a), the two triangles in the order above; int32 vertex numbers local to the volume, never -1.
 *   out_vertices fp32 [max_vertices, 3], out_faces int32 [max_faces, 3], out_cells (nullable) int32 [max_vertices]: each vertex's
 *   linear cell index.  out_v_offsets, out_f_offsets DEVICE int64 [batch + 1]: volume b's rows are offsets[b] .. offsets[b + 1] - 1;
 *   they always hold the TRUE counts.  max_vertices and max_faces (0 .. 2^40) are HOST capacities over the whole batch: a row at or
 *   beyond its capacity is not written, a triangle is written whole or not at all.  out_vertices, out_faces NULL: that output is not
 *   written; with both (and out_cells) NULL the call only counts.  Nothing outside these rows is written.
 * Launches (surface_nets.hip): the volume is read once into one 64-bit word of INSIDE bits per run of 64 nodes along z; one lane per
 * word makes the active mask (any & ~all over the four rows' words and their one-bit shifts), the face masks (XORs) and their
 * popcounts; the two block scans of the ragged-cloud calls run over the words; one wave per word emits the vertices (eight loads
 * per ACTIVE cell) and one the triangles (a vertex number is its word's base plus a popcount), visiting only the words that hold
 * something.  One stream, no atomics, no kernel waits on another workgroup, every loop bounded by a constant; every row index derived
 * from the scratch is checked against the capacity.
 * scratch: rald_post_surface_scratch_bytes of the same batch and dims (about half a byte per node), 16-byte aligned, never NULL;
 * -1 (and rald_last_error) for sizes the call refuses.  Every invalid argument is refused with a status before any GPU work. */
int64_t rald_post_surface_scratch_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t nz);
int rald_post_surface_nets(const float* volume, int32_t batch, const int32_t* dims3_host, const float* lo3_host, const float* spacing3_host,
                           float iso, float* out_vertices, int64_t* out_v_offsets, int64_t max_vertices, int32_t* out_faces,
                           int64_t* out_f_offsets, int64_t max_faces, int32_t* out_cells, void* scratch, int64_t scratch_bytes, void* stream);
/* pred = logits >= 0; accuracy[b] = mean(pred == labels); iou[b] = |pred & labels| / |pred | labels| + 1e-5 */
int rald_post_iou(const float* logits, const float* labels, int32_t batch, int64_t n_queries, float* out_accuracy, float* out_iou, void* stream);

/* ------------------------------------------------------------------------------------------
 * Query generation + refine on the device (the host numpy code between model.sample and vae.decode in
 * engine_generation.evaluate, :250-300).  Random draws are caller-supplied DEVICE arrays so that the
 * host mirror can replay numpy's global-RNG stream (bit-identical queries) or use a device generator.
 * ---------------------------------------------------------------------------------------- */
/* generate_query_points (utils/utils.py:147-175): u3n = [3,n] float64 uniforms in numpy's draw order
 * (all x, then all y, then all z); out[i,a] = float32(lo_a + (hi_a - lo_a) * u[a,i]), box = [-1,1]^3
 * (anisotropic) or +-scale_a/max_scale (isotropic). */
int rald_query_uniform(const double* u3n, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy,
                       float* out_queries, void* stream);
/* the use_cart_query branch (engine_generation.py:251-256): uniform in the cartesian box ->
 * inverse_norm_points(pc_range_cart) -> cartesian2polar (dataset_preprocessor/lidar.py:49-55) ->
 * norm_points(pc_range) -> remove_points_outside_fov (utils/utils.py:106-112), float64 throughout,
 * float32 on output; survivors keep their order, *out_count (device int64) = their number.
 * scratch: rald_post_scratch_bytes(n). */
int rald_query_uniform_cart(const double* u3n, int64_t n, const double* pc_range_cart6_host, const double* pc_range6_host,
                            int32_t norm_anisotropy, int32_t norm_isotropy, float* out_queries, int64_t* out_count, void* scratch,
                            void* stream);
/* norm_points (utils/utils.py:77-104) of a float32 array */
int rald_query_norm_points(const float* points, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy,
                           float* out_points, void* stream);
/* The nodes of a regular grid, the positions rald_post_surface_nets gives its volume: x-planes i0 .. i0 + ni - 1 (inside 0 .. nx - 1) as
 * out fp32 [ni * ny * nz, 3], z fastest; node (i, j, k) at fl(lo_a + fl((float)i_a * h_a)) per axis, fp32 without contraction.  lo3 finite,
 * spacing3 finite and > 0, dims3 each 2 .. 1024, all HOST arrays. */
int rald_query_grid(const float* lo3_host, const float* spacing3_host, const int32_t* dims3_host, int32_t i0, int32_t ni, float* out_points,
                    void* stream);
/* aug_query_helper (datasets/utils/query_helper.py:3-42) [+ norm_points when normalise != 0, as
 * engine_generation.py:292-297 does]: out [aug_num,3] = the first min(n_helper, aug_num) helper points, then
 * for g < aug_num - n_helper: clip(helper[sel_index[g]] + (2*u_bias[g,:]-1) * voxel_size * aug_scales[g]).
 * sel_index / aug_scales: int64 [aug_num - n_helper]; u_bias: float64 [aug_num - n_helper, 3] (may be NULL when
 * n_helper >= aug_num). */
int rald_query_refine(const float* helper_points, int64_t n_helper, int64_t aug_num, const int64_t* sel_index, const int64_t* aug_scales,
                      const double* u_bias, const double* pc_range6_host, const double* voxel_size3_host, int32_t norm_anisotropy,
                      int32_t norm_isotropy, int32_t normalise, float* out_points, void* stream);
/* rald_query_refine for a ragged batch of helper points (points [n_total,3], offsets DEVICE int64 [batch+1]): a sample with N_b > 0
 * points gets aug_num rows - its first min(N_b, aug_num) points, then row j >= N_b from draw g = j - N_b of ITS rows of the draws
 * (sel_index / aug_scales int64 [batch,aug_num], u_bias float64 [batch,aug_num,3]; sel_index NULL: the point min(floor(u_sel[b,g] *
 * N_b), N_b - 1) in float64, u_sel float64 [batch,aug_num] in [0,1)) - and a sample without points gets none.  out_queries
 * [batch*aug_num,3] holds the samples packed, out_offsets (DEVICE int64 [batch+1]) their rows.  No host read. */
int rald_query_refine_ragged(const float* points, const int64_t* offsets, int32_t batch, int64_t aug_num, const int64_t* sel_index,
                             const double* u_sel, const int64_t* aug_scales, const double* u_bias, const double* pc_range6_host,
                             const double* voxel_size3_host, int32_t norm_anisotropy, int32_t norm_isotropy, int32_t normalise,
                             float* out_queries, int64_t* out_offsets, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer step of train_one_epoch (engine_generation.py:96-110) on FLAT fp32 storage: the model's
 * parameters, gradients, Adam moments and the EMA copy are five arrays with one layout.
 *   clip_grad_norm_ (utils/misc.py:262) -> torch.optim.AdamW(lr) (main_generation.py:161; betas 0.9/0.999,
 *   eps 1e-8, weight_decay 0.01 defaults) -> update_ema(rate 0.999) (engine_generation.py:29-40, :110)
 * ---------------------------------------------------------------------------------------- */
/* *out_sumsq (device double) = sum g^2 (fp64 accumulation) */
int rald_optim_grad_sumsq(const float* grads, int64_t n, double* out_sumsq, void* stream);
/* out[0] = total_norm = sqrt(*sumsq) * pre_scale; out[1] = pre_scale * min(max_norm / (total_norm + 1e-6), 1)
 * (max_norm <= 0: no clipping).  pre_scale folds the 1/world of a SUM all-reduce.  Device in, device out: no sync. */
int rald_optim_clip_coef(const double* sumsq, float pre_scale, float max_norm, float* out_norm_coef, void* stream);
/* one fused pass: g *= *grad_scale (device scalar, NULL = 1); p *= 1 - lr*wd; m, v updates; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps);
 * ema = ema*rate + p*(1-rate) when ema_params != NULL.  step counts from 1.  write_back_grads != 0 stores the scaled gradient. */
int rald_optim_adamw_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema_params, int64_t n,
                         const float* grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                         double ema_rate, int32_t write_back_grads, void* stream);
/* update_ema alone (the reference also runs it on gradient-accumulation iterations) */
int rald_optim_ema(float* ema_params, const float* params, int64_t n, double rate, void* stream);

/* ColoRadarDataset.process_radar_data (datasets/aligned_coloradar/Coloradar_dataset.py:432-475): raw cube
 * [B,R,A,E,raw_channels] (intensity dB, doppler, ..., validity mask last; the .bin layout of load_radarcube
 * :420-430) -> the network's input [B,R,tgt_A,tgt_E,2]: intensity clipped to [0,max] / max, doppler * mask
 * / max_dopp, bilinear (align_corners=True) upsampling over (A,E). */
int rald_radar_cube_prepare(const float* raw, int32_t batch, int32_t R, int32_t A, int32_t E, int32_t raw_channels, int32_t tgt_A,
                            int32_t tgt_E, int32_t norm_intensity, float max_intensity, int32_t norm_dopp, float max_dopp, float* out,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Radar front end (dataset_preprocessor/radar.py:64-76 load_radar_data + utils/radar_preprocessing.py:6-62 RAEIVVmap):
 * raw ADC frames -> RAEIVV cubes [R = range_fft][A = angle_fft][E = elevation_fft][3] (intensity dB, velocity, validity 0/1).
 * range_fft / doppler_fft: powers of two in [2, 256]; angle_fft / elevation_fft: [1, 64].  crop_low / crop_high are the
 * fractions of range bins zeroed at the head / tail; int(range_fft * crop_high) must be >= 1 (the reference's [-0:] slice
 * would zero every bin).  Everything is checked, and the host tables built, at create.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t ntx, nrx, n_chirps, n_samples;
    int32_t range_fft, doppler_fft, angle_fft, elevation_fft;
    double crop_low, crop_high;
} rald_radar_dsp_config;
typedef struct rald_radar_dsp rald_radar_dsp;
/* tx_layout [ntx][3], rx_layout [nrx][3] int32 rows {data index, azimuth, elevation} in half wavelengths (config/antenna_array.txt);
 * vbins [n_vbins] = the velocity reported for Doppler bin d (the reference's vbins; n_vbins >= doppler_fft). */
int rald_radar_dsp_create(const rald_radar_dsp_config* cfg, const int32_t* tx_layout, const int32_t* rx_layout, const double* vbins,
                          int32_t n_vbins, rald_radar_dsp** out);
void rald_radar_dsp_destroy(rald_radar_dsp* h);
/* device workspace rald_radar_dsp_run needs for `batch` frames (host arithmetic; -1 on a bad configuration) */
int64_t rald_radar_dsp_workspace_bytes(const rald_radar_dsp_config* cfg, int32_t batch);
/* frames [batch][ntx][nrx][n_chirps][n_samples][2] (I, Q): input_kind 0 = int16, the frame's complex mean removed (radar.py:75);
 * input_kind 1 = fp32, used as given.  out: fp32 [batch][R][A][E][3].  A frame's result does not depend on the batch. */
int rald_radar_dsp_run(const rald_radar_dsp* h, const void* frames, int32_t input_kind, int32_t batch, float* out, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Helper points: RAEIVV intensity cubes -> CFAR query points (dataset_preprocessor/cache_test_cfar.py:68-93:
 * rae_interpo, weighted_allocation, RA2DDetectorTensor, cube_idx2coord, filter_points_polar)
 * ---------------------------------------------------------------------------------------- */
typedef struct rald_radar_points_config {
    int32_t in_r, in_a, in_e, in_channels;   /* source cube; channel 0 is read */
    int32_t tgt_r, tgt_a, tgt_e;             /* trilinear target (align_corners=False); tgt_a * tgt_e <= 32768 */
    int64_t num_points;                      /* 1 .. tgt_r*tgt_a*tgt_e (and <= INT32_MAX) */
} rald_radar_points_config;
typedef struct rald_radar_points rald_radar_points;
/* axis_r / axis_a / axis_e: float32 coordinate of each target index (tgt_r / tgt_a / tgt_e entries: range in m, azimuth and
 * elevation in degrees); keep_r / keep_a / keep_e: nonzero where that coordinate passes the FOV filter. */
int rald_radar_points_create(const rald_radar_points_config* cfg, const float* axis_r, const float* axis_a, const float* axis_e,
                             const uint8_t* keep_r, const uint8_t* keep_a, const uint8_t* keep_e, rald_radar_points** out);
void rald_radar_points_destroy(rald_radar_points* h);
/* device workspace rald_radar_points_run needs for `batch` frames (host arithmetic; -1 on a bad configuration) */
int64_t rald_radar_points_workspace_bytes(const rald_radar_points_config* cfg, int32_t batch);
/* cubes fp32 [batch][in_r][in_a][in_e][in_channels].  Per frame, num_points voxels of the upsampled intensity are chosen: slice r
 * gets floor(num * s_r / sum s) (in double; the surplus to the first slice of largest sum s_r), and takes its largest values, ties
 * at the k-th value by lowest flat index a * tgt_e + e.  Output order: slices ascending, then value descending, then flat index
 * ascending.  points [batch][num_points][3] polar (r, az deg, el deg) of the chosen voxels the keep masks pass, compacted: the
 * first counts[b] rows are valid.  counts[b] = -1 when the frame's total is not positive and finite, -2 when a slice would need
 * more points than it has voxels; the other frames are still written.  peaks [batch][num_points][3] int32 (r, a, e) and
 * intensities [batch][num_points], before the filter and in output order, are optional (NULL).  A frame's output does not depend
 * on the batch. */
int rald_radar_points_run(const rald_radar_points* h, const float* cubes, int32_t batch, float* points, int32_t* counts, int32_t* peaks,
                          float* intensities, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LiDAR front end: raw scans -> cropped points (dataset_preprocessor/lidar.py:123-194), voxels (datasets/utils/voxelize.py, spconv
 * Point2VoxelCPU3d) and occupancy queries (datasets/aligned_coloradar/Coloradar_dataset.py:70-135, :237-418).  Frames are packed
 * [total][F] float32 with HOST int64 offsets [batch + 1] (offsets[0] = 0, non-decreasing, frames below 2^31 points), checked before
 * any launch.  A frame's outputs do not depend on the batch.
 * ---------------------------------------------------------------------------------------- */
typedef struct rald_lidar_config {
    double pc_range[6];                      /* lo x y z, hi x y z (dataset.lidar.pc_range; r / az / el in view-cone mode) */
    double voxel_size[3];                    /* > 0; grid = round((hi - lo) / voxel_size), at most 2^31 - 1 cells in all */
    int32_t max_points_per_voxel, max_voxels, num_point_features;
    int32_t view_cone_mode, norm_anisotropy, norm_isotropy;
    double extrinsic[16];                    /* T_RADAR_TO_LIDAR, row-major (dataset_preprocessor/constants.py:602) */
    double fov[6];                           /* r lo, r hi, az lo, az hi, el lo, el hi in degrees, inclusive (lidar.py:172-177) */
} rald_lidar_config;
typedef struct rald_lidar rald_lidar;
/* rejects non-positive voxel sizes, empty axes and grids over 2^31 cells */
int rald_lidar_create(const rald_lidar_config* cfg, rald_lidar** out);
void rald_lidar_destroy(rald_lidar* h);
/* device workspace any of the three calls below needs for `batch` frames of `total_points` points (host arithmetic; -1 on a bad
 * configuration) */
int64_t rald_lidar_workspace_bytes(const rald_lidar_config* cfg, int32_t batch, int64_t total_points);
/* lidar.py:170-182 per point, in float64: remove_empty_points, [x y z 1] @ T.T, cartesian2polar, filter_points_polar, polar2cartesian,
 * rounded once to float32.  points [total][in_stride] (x, y, z first); out [total][3]: frame b's survivors, in input order, at rows
 * offsets[b] .. offsets[b] + counts[b]. */
int rald_lidar_crop(const rald_lidar* h, const float* points, int32_t in_stride, const int64_t* offsets, int32_t batch, float* out,
                    int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
/* Point2VoxelCPU3d (voxelize.py:559-576): cell c = floor((p - lo) / v) in float32, outside when c < 0 or c >= grid; voxels are numbered
 * by their first point; a new voxel beyond max_voxels is dropped, points of kept voxels still count; a voxel keeps its first
 * max_points_per_voxel points in input order.  points [total][F]; counts [batch] (nullable): frame b is its first
 * min(counts[b], offsets[b+1] - offsets[b]) rows.  to_polar: first convert the points to float32 polar as numpy's cartesian2polar
 * does on float32 (Coloradar_dataset.py:87-88; F must be 3) into polar_out [total][3].  Outputs per frame b, rows past
 * voxel_counts[b] unspecified: voxels [batch][max_voxels][max_points_per_voxel][F] zero-filled (nullable), coords
 * [batch][max_voxels][3] int32 in z, y, x order, num_points [batch][max_voxels], kept_keys [batch][max_voxels] the linear cells
 * (x * Gy + y) * Gz + z of the kept voxels in ascending order (the input of rald_lidar_queries). */
int rald_lidar_voxelize(const rald_lidar* h, const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch,
                        int32_t to_polar, float* polar_out, float* voxels, int32_t* coords, int32_t* num_points, int32_t* kept_keys,
                        int32_t* voxel_counts, void* workspace, int64_t workspace_bytes, void* stream);
/* transform_voxels_to_query_points + get_empty_voxel_centers + norm_points (Coloradar_dataset.py:237-294, :335-418) from drawn inputs.
 * points [total][3] (what the samples index), sample_idx [batch][S]; in-voxel rows s < in_num: centre(coords[voxel_idx]) +
 * float32(u_in), label 1; the other rows: centre of the empty_rank-th empty cell in row-major (x, y, z) order + float32(u_out),
 * label 0.  u_in [batch][in_num][3], voxel_idx [batch][in_num], u_out [batch][S - in_num][3], empty_rank [batch][S - in_num].  Out:
 * lidar_points, query_points [batch][S][3] normalised, query_labels [batch][S] float32.  An index out of range gives NaN rows. */
int rald_lidar_queries(const rald_lidar* h, const float* points, const int64_t* offsets, int32_t batch, int32_t num_samples,
                       int32_t in_num, const int64_t* sample_idx, const double* u_in, const int64_t* voxel_idx, const double* u_out,
                       const int64_t* empty_rank, const int32_t* coords, const int32_t* kept_keys, const int32_t* voxel_counts,
                       float* lidar_points, float* query_points, float* query_labels, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Kernel-level entry points (what the parity tests and microbenchmarks drive directly)
 * ---------------------------------------------------------------------------------------- */
/* C[b][m][n] = alpha * sum_k A[b][m][k]*B[b][n][k] (+bias[n]); A,B bf16 (K contiguous).
 * epilogue: 0 bf16 out, 1 f32 out, 2 f32 C += result, 3 GEGLU (packed B rows, bf16 out, N/2 cols) */
int rald_op_gemm_nt(const void* A, int64_t lda, int64_t strideA, const void* B, int64_t ldb, int64_t strideB,
                    void* C, int64_t ldc, int64_t strideC, const float* bias, int32_t M, int32_t N, int32_t K,
                    int32_t batch, float alpha, int32_t epilogue, void* stream);
/* rald_op_gemm_nt with an inner batch (attention heads): grid z = batch * batch2, operand offset =
 * b1 * stride + b2 * stride2 */
int rald_op_gemm_nt2(const void* A, int64_t lda, int64_t strideA, int64_t strideA2, const void* B, int64_t ldb, int64_t strideB, int64_t strideB2,
                     void* C, int64_t ldc, int64_t strideC, int64_t strideC2, const float* bias, int32_t M, int32_t N, int32_t K, int32_t batch,
                     int32_t batch2, float alpha, int32_t epilogue, void* stream);
/* Test entry of the 256 x 256 LDS-DMA tiles: one problem (no batch) with M, N multiples of 256, K a multiple of 64, epilogue 0 (bf16;
 * alpha applies to columns n < alpha_ncols only) or 3 (GEGLU, packed bias required), launched whatever the tile count:
 * persistent = 1 the persistent tile loop on at most max_workgroups workgroups (and at most one per CU), persistent = 0 the one-tile
 * kernel.  The two are bit-identical; rald_op_gemm_nt picks between them by tile count. */
int rald_op_gemm_nt_256(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const float* bias, int32_t M, int32_t N,
                        int32_t K, float alpha, int32_t alpha_ncols, int32_t epilogue, int32_t persistent, int32_t max_workgroups, void* stream);
/* rald_op_gemm_nt_256 with a batch: entry b reads A + b strideA and B + b strideB (elements; 0 = shared by every entry) and writes
 * C + b strideC (at least one whole output apart).  epilogue 4 (softmax over every aligned group of 64 output columns of alpha * acc, in
 * exp2 units; no bias, alpha_ncols >= N) is accepted beside 0 and 3.  batch2 must be 1: the tiles have no inner batch.  The persistent
 * tile loop takes a batch for epilogue 4 only (tile index over batch entry, m-tile, n-tile); batches of 0 and 3 run with persistent = 0.
 * Every argument is checked on the host before the first HIP call. */
int rald_op_gemm_nt_256_batched(const void* A, int64_t lda, int64_t strideA, const void* B, int64_t ldb, int64_t strideB, void* C, int64_t ldc,
                                int64_t strideC, const float* bias, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t batch2, float alpha,
                                int32_t alpha_ncols, int32_t epilogue, int32_t persistent, int32_t max_workgroups, void* stream);
/* Backward building blocks of the transformer block (what autograd derives for
 * models_radar_generation.py:35-169).  dX = dY.W and dW = dY^T.X run on rald_op_gemm_nt with transposed operands. */
/* Weight gradient of a Linear without transposed copies (rald_amd/csrc/gemm_tn.hip): C[n1][n2] += sum_m A[m][n1] B[m][n2] for row-major bf16
 * A [M, N1] (= dY) and B [M, N2] (= X), fp32 C accumulated into; colsum (nullable) [N1] += column sums of A (the bias gradient).
 * N1, N2, lda, ldb multiples of 8. */
int rald_op_gemm_tn(const void* A_bf16, int64_t lda, const void* B_bf16, int64_t ldb, float* C, int64_t ldc, float* colsum, int32_t M, int32_t N1,
                    int32_t N2, void* workspace, int64_t workspace_bytes, void* stream);
/* Weight gradient of a 3x3x3 Conv3d (Encoder :216-241 under autograd) with the patch matrix never formed: dW [Cout][Cin][27] +=
 * sum over output voxels of dy[v][co] x[v*stride - pad + offset(tap)][ci] (zero outside the volume); dbias (nullable) += column sums
 * of dy.  dy [B*OD*OH*OW][Cout] bf16, x [B][ID][IH][IW][Cin] bf16 channels-last, OD = ID / stride ... */
int rald_op_conv3d_wgrad(const void* dy_bf16, const void* x_bf16, float* dW, float* dbias, int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin,
                         int32_t Cout, int32_t stride, int32_t pad, void* workspace, int64_t workspace_bytes, void* stream);
/* workspace of the two weight-gradient products above: null = fp32 atomics into C / dW (and colsum / dbias).  Otherwise a caller-owned
 * workspace of _workspace_bytes(...) bytes (16-byte aligned; 0 = this shape keeps the atomic form): every row / voxel range stores its partial
 * result there and a second launch adds the ranges IN ORDER: bit-reproducible run to run, and several times faster for the convolution below
 * full resolution, whose atomics scatter over the parameter's tap-innermost layout. */
int64_t rald_op_gemm_tn_workspace_bytes(int32_t M, int32_t N1, int32_t N2);
int64_t rald_op_conv3d_wgrad_workspace_bytes(int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad);
/* Which kernel rald_op_conv3d_wgrad runs a shape on and how it cuts the voxels: the plan function of the launch itself (pure host arithmetic,
 * no HIP call, works where no GPU is visible).  Returns 1 for the line-staged kernel (stride 1 / pad 1, or stride 2 / pad 0 on even dims; channel
 * counts multiples of 64, output width a power of two in 4..64, whole 64-voxel steps) and 0 for the generic row-contracting kernel (narrow
 * for Cout <= 64).  *ranges_out (nullable) = the voxel ranges that do work (one slab each in the workspace form); *per_range_out (nullable) =
 * the 64-voxel steps of one range (line) or its rows (generic; for Cout > 64 the workspace form's - the atomic form cuts finer).
 * -1 (and rald_last_error) for a shape rald_op_conv3d_wgrad refuses. */
int rald_op_conv3d_wgrad_route(int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad,
                               int32_t* ranges_out, int32_t* per_range_out);
/* conv_in (one input channel) weight gradient, first half: the 27-neighbourhood of channel 0 of cube [B][D][H][W][cube_ch] fp32 per voxel as one
 * bf16 row of 32 (taps kd*9 + kh*3 + kw, zero outside the volume, 5 zero pads); dW = rald_op_gemm_tn(dy, patches). */
int rald_op_patches27(const float* cube, int32_t cube_ch, void* out_bf16, int32_t B, int32_t D, int32_t H, int32_t W, void* stream);
/* in [batch][batch2][rows][cols] (f32 or bf16) -> out [batch][batch2][cols][rows] bf16 */
int rald_op_transpose(const void* in, int32_t in_is_bf16, int64_t ld_in, int64_t stride_in, int64_t stride_in2, void* out_bf16, int64_t ld_out,
                      int64_t stride_out, int64_t stride_out2, int32_t rows, int32_t cols, int32_t batch, int32_t batch2, void* stream);
/* AdaLayerNorm :119-131 (add_one = 1) / LayerNorm (add_one = 0, scale = weight) backward, D = 512:
 * dx += ..., dscale[g] += sum_rows dh * xhat, dshift[g] += sum_rows dh  (g = row / rows_per_group, stride gstride);
 * dx_bf16_out (nullable) receives the updated dx as bf16 [rows][512] (what the next weight-/input-gradient GEMMs of the block read) */
int rald_op_ln_mod_bwd(const float* x, const float* dh, const float* scale, int64_t gstride, int32_t rows_per_group, float add_one, float eps,
                       int64_t rows, int32_t D, float* dx_accum, void* dx_bf16_out, float* dscale_accum, float* dshift_accum, void* stream);
/* GEGLU :88-95 in the natural layout u = [a | g] (2*inner columns): hid = a * gelu_erf(g); and its backward */
int rald_op_geglu_fwd(const void* u_bf16, void* hid_bf16, int64_t M, int32_t inner, void* stream);
int rald_op_geglu_bwd(const void* u_bf16, const void* dhid_bf16, void* du_bf16, int64_t M, int32_t inner, void* stream);
/* bias gradient: out[n] += sum_m X[m][n] */
int rald_op_colsum(const void* X, int32_t is_bf16, int64_t ld, int64_t M, int32_t N, float* out_accum, void* stream);
/* attention backward, element-wise parts: lse[r] = log sum_c exp(scale*S[r][c]); delta[b][h][q] = <dO, O> over head h of row m = b*nq + q;
 * P = exp(scale*S - lse[i]), dS = P*(dP - delta[i])*scale with i = row (by_col 0) or column (by_col 1) */
int rald_op_row_lse(const float* S, int64_t rows, int32_t cols, float scale, float* lse, void* stream);
int rald_op_rowdot_heads(const void* dO_bf16, const void* O_bf16, int64_t M, int32_t heads, int32_t nq, float* delta, void* stream);
int rald_op_attn_bwd_elem(const float* S, const float* dP, const float* lse, const float* delta, int64_t batch, int32_t R, int32_t Ccols,
                          int64_t vbatch_stride, int32_t vstride, float scale, int32_t by_col, void* P_bf16, void* dS_bf16, void* stream);
/* thin fp32 products of the training step (timestep MLP, AdaLN linears, proj_in/out and their gradients):
 * C[m][n] += alpha * sum_k A(m,k)*B(n,k); A(m,k) = A[m*lda+k] or (trans_a) A[k*lda+m]; B(n,k) = B[n*ldb+k] or (trans_b) B[k*ldb+n] */
int rald_op_sgemm_acc(const float* A, int64_t lda, int32_t trans_a, const float* B, int64_t ldb, int32_t trans_b, float* C, int64_t ldc, int32_t M,
                      int32_t N, int32_t K, float alpha, void* stream);
int rald_op_silu_fwd(const float* x, float* y, int64_t n, void* stream);
int rald_op_silu_bwd(const float* x_pre, const float* dy, float* dx, int64_t n, void* stream);
/* PositionalEmbedding :20-33: out [n, channels] = cat[cos, sin](outer(t, freqs)) */
int rald_op_posemb(const float* t, float* out, int32_t n, int32_t channels, void* stream);
/* EDMLoss :283-295 over EDMPrecond.forward's output mix :422-430: coef3[b] = {c_skip, c_out, weight};
 * D = c_skip*x_noised + c_out*F; *loss = mean(weight*(D - y)^2) (device double); dF = dloss/dF; D_out optional */
int rald_op_edm_loss_grad(const float* F, const float* x_noised, const float* y, const float* coef3, int64_t per_sample, int64_t total, float* dF,
                          float* D_out, double* loss, void* stream);
/* Radar-spectrum encoder at op level (model/models_radar_encoder.py:29-241), channels-last activations
 * [b][d][h][w][c]: the forward kernels of rald_radar_encode plus the backward building blocks (the shipped
 * configuration trains the encoder jointly with the denoiser). */
/* Conv3d k3 as implicit GEMM: in bf16 [B][ID][IH][IW][Cin], w packed bf16 [Cout][27][Cin] (rald_op_conv_pack_weights),
 * out f32 [B][ID/s][IH/s][IW/s][Cout] = conv + bias (+ resid).  Cin % 64 == 0, Cout % 4 == 0, stride 1|2.
 * Exactly one of out and out_bf16 is non-null: out_bf16 takes the result as bf16 without a residual (the data-gradient convolutions of the
 * training step, whose only reader is the GroupNorm backward with da_is_bf16 = 1). */
int rald_op_conv3d(const void* in_bf16, const void* w_packed_bf16, const float* bias, const float* resid, float* out, void* out_bf16, int32_t B,
                   int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad, void* stream);
/* Which engine a Conv3d shape runs on: the library's one engine-choice function (pure host arithmetic, no HIP call, works where no GPU is
 * visible).  Returns 0 igemm (gathers per tap; any stride / width), 1 line (stride 1, pad 1, W in {8,16,32}, M % 128 == 0), 2 plane and
 * 3 persistent plane (the 64-input-channel full-resolution levels), 4 igemm with split K + reduce pass (allow_split = 1 only: few tiles x
 * long K, as the encoder runs its 512- and 64-voxel levels); *splits_out (nullable) = the number of k-ranges, 1 when not split.
 * -1 (and rald_last_error) for a shape rald_op_conv3d_full refuses. */
int rald_op_conv3d_route(int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad, int32_t allow_split,
                         int32_t* splits_out);
/* rald_op_conv3d with every field of the kernels' argument block reachable (tests): allow_split = 0 is rald_op_conv3d exactly; 1 takes the
 * route the encoder takes, i.e. where rald_op_conv3d_route reports 4 the k-ranges meet as fp32 partial sums in split_workspace (caller-owned,
 * 16-byte aligned, at least splits * M * Cout * 4 bytes, M = B * output voxels) and a second launch adds them in order with bias and residual.
 * gn_part (nullable): [B * So / 128][32][2] doubles = {sum, sum of squares} per 128-voxel tile and GroupNorm group of the OUTPUT, written by
 * the convolution epilogue (So = output voxels per sample, So % 128 == 0, Cout in {64, 128, 256}; not where the route splits).
 * resid == out is allowed (the in-place residual of a ResnetBlock: every element is read and then written by the same thread).
 * out_bf16 excludes out, resid and a split route. */
int rald_op_conv3d_full(const void* in_bf16, const void* w_packed_bf16, const float* bias, const float* resid, float* out, void* out_bf16,
                        double* gn_part, void* split_workspace, int64_t split_workspace_bytes, int32_t allow_split, int32_t B, int32_t ID,
                        int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad, void* stream);
/* stats [B][32][2] = per sample the sum, in a fixed order, of its nblk partial slots part[b * nblk + k][32][2] (what rald_op_conv3d_full's
 * gn_part holds with nblk = So / 128): the statistics rald_op_groupnorm_apply normalises with */
int rald_op_gn_finish(const double* part, double* stats, int32_t B, int32_t nblk, void* stream);
/* The radar decoder's data movement: nearest-neighbour x2 of x f32 [B][D][H][W][C] -> bf16 [B][2D][2H][2W][C] (C % 4 == 0);
 * z f32 [rows][zc] -> bf16 [rows][64], zero beyond zc (1 <= zc <= 64). */
int rald_op_upsample2_cast(const float* x, void* y_bf16, int32_t B, int32_t D, int32_t H, int32_t W, int32_t C, void* stream);
int rald_op_pad_cast64(const float* z, void* y_bf16, int64_t rows, int32_t zc, void* stream);
/* The tokeniser half of rald_radar_tokens without the encoder (EDMPrecond.process_radar_cond :387-407): z f32 [B][R][A][E][zc] on the token
 * grid -> tokens f32 [B][R*A*E][C] = z . Wp[C][zc]^T + bp + r_emb[r] + a_emb[a] + e_emb[e] (embeddings [R|A|E][C]); zc <= 64, B <= 65535. */
int rald_op_radar_tokens(const float* z, const float* Wp, const float* bp, const float* r_emb, const float* a_emb, const float* e_emb, float* tokens,
                         int32_t B, int32_t R, int32_t A, int32_t E, int32_t zc, int32_t C, void* stream);
/* W [Cout][Cin][27] f32 (the parameter) -> packed bf16: dgrad = 0: [Cout][27][pad_to >= Cin]; dgrad = 1: the flipped,
 * transposed weights [Cin][27][pad_to >= Cout] that make rald_op_conv3d map dY to dX */
int rald_op_conv_pack_weights(const float* W, void* out_bf16, int32_t Cout, int32_t Cin, int32_t pad_to, int32_t dgrad, void* stream);
/* Normalize :9-12 (GroupNorm 32 groups, eps 1e-6) [+ swish :5-7]: y bf16; stats: B*64*(1 + ceil(S/512)) doubles - the first [B][32][2] =
 * {sum, sumsq} are kept for the backward, the rest is scratch for the per-block partials of the deterministic (atomic-free) reduction */
int rald_op_groupnorm(const float* x, const float* gamma, const float* beta, void* y_bf16, double* stats, int32_t B, int32_t S, int32_t C,
                      int32_t swish, void* stream);
/* its backward: da = gradient w.r.t. the (activated) output, fp32 or bf16 (da_is_bf16 = 1); dx written or accumulated; dx_bf16 (nullable)
 * receives the resulting dx rounded to bf16 (what the convolution gradients of the next layer read), and dx may then be null (not with
 * accumulate); dgamma/dbeta accumulated; gsum_scratch: 8-byte aligned, rald_op_groupnorm_bwd_scratch_bytes(B, S, C) bytes (group sums + the
 * per-workgroup partial sums of the atomic-free, bit-reproducible reduction) */
int64_t rald_op_groupnorm_bwd_scratch_bytes(int32_t B, int32_t S, int32_t C);
int rald_op_groupnorm_bwd(const float* x, const double* stats, const float* gamma, const float* beta, const void* da, int32_t da_is_bf16, float* dx,
                          void* dx_bf16, float* dgamma, float* dbeta, double* gsum_scratch, int32_t B, int32_t S, int32_t C, int32_t swish,
                          int32_t accumulate, void* stream);
/* rald_op_groupnorm's normalisation alone, from the [B][32][2] statistics a forward call left (the training backward re-creates activations) */
int rald_op_groupnorm_apply(const float* x, const double* stats, const float* gamma, const float* beta, void* y_bf16, int32_t B, int32_t S, int32_t C,
                            int32_t swish, void* stream);
/* conv_in (Cin = 1 read in place from channel 0 of the cube) */
int rald_op_conv_in(const float* cube, int32_t cube_ch, int32_t Cin, const float* W, const float* bias, float* out, int32_t B, int32_t D, int32_t H,
                    int32_t Wd, int32_t Cout, void* stream);
/* x [M][C] f32 -> bf16 [M][Cpad] zero-filled;  dY [B][OD][OH][OW][C] f32 -> bf16 on the even positions of a 2x grid (Downsample dgrad) */
int rald_op_pad_channels(const float* x, void* out_bf16, int64_t M, int32_t C, int32_t Cpad, void* stream);
int rald_op_zero_insert2(const float* dy, void* out_bf16, int32_t B, int32_t OD, int32_t OH, int32_t OW, int32_t C, void* stream);
int rald_op_rowdot(const void* a_bf16, const void* b_bf16, int64_t M, int32_t C, float* out, void* stream);
int rald_op_softmax_rows(const float* S, int64_t ld_s, void* P_bf16, int64_t ld_p, int32_t rows, int32_t n, void* stream);
/* Small-batch fused attention sub-blocks (rald_amd/csrc/attn_small.hip; CrossAttention :55-76 + the to_out Linear).
 * _self_proj: qkv [batch*n_latents][ld] bf16 = q (pre-multiplied by scale*log2e) | k | v of a fused projection, 8 heads x 64;
 *   part[h][row][512] = attention output of head h times Wo[:, 64h:64h+64]^T (fp32 partial of to_out).
 * _q2_proj: h [M][512] bf16 -> to_q (Wq, scaled by qscale) -> attention over 64 cached condition tokens (Kc[b*strideK + key*ldk +
 *   64h + d], Vt[b*strideVt + (64h + d)*ldvt + key]) -> part likewise.
 * _reduce_resid_ln: x[M][512] += bias + sum_s part[s] (fixed order); h = LN(x)*(add_one + g) + b as bf16 when h is given. */
int rald_op_attn_self_proj(const void* qkv_bf16, int64_t ld, const void* Wo_bf16, float* part, int32_t n_latents, int32_t heads, int32_t batch,
                           void* stream);
int rald_op_xattn_q2_proj(const void* h_bf16, const void* Wq_bf16, const void* Kc_bf16, int64_t ldk, int64_t strideK, const void* Vt_bf16,
                          int64_t ldvt, int64_t strideVt, const void* Wo_bf16, float* part, int32_t M, int32_t n_latents, int32_t heads,
                          int32_t n_keys, float qscale, void* stream);
/* The same two sub-blocks and the slab reduction with the slab type as an argument (tests): part_f16 != 0 = the slabs are fp16 holding
 * 2^-6 x the value, saturated at +-65504 (+-4.19e6 in value), as the models run these kernels; `part` then points at halves and
 * slab_stride counts halves.  fp16 slabs are reduced in eights (one per head) or fours.  rald_debug_f16_saturation_attn: the number of
 * 4-element groups the two sub-blocks clamped since the last reset (reset != 0 clears it); synchronises the device; -1 on error. */
int rald_op_attn_self_proj_slabs(const void* qkv_bf16, int64_t ld, const void* Wo_bf16, void* part, int32_t n_latents, int32_t heads, int32_t batch,
                                 int32_t part_f16, void* stream);
int rald_op_xattn_q2_proj_slabs(const void* h_bf16, const void* Wq_bf16, const void* Kc_bf16, int64_t ldk, int64_t strideK, const void* Vt_bf16,
                                int64_t ldvt, int64_t strideVt, const void* Wo_bf16, void* part, int32_t M, int32_t n_latents, int32_t heads,
                                int32_t n_keys, float qscale, int32_t part_f16, void* stream);
int rald_op_reduce_resid_ln_slabs(const void* part, int32_t slabs, int64_t slab_stride, const float* bias, float* x, void* h_bf16, int32_t M,
                                  const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps, int32_t part_f16,
                                  void* stream);
int64_t rald_debug_f16_saturation_attn(int32_t reset);
/* The denoiser's first and last layers (LatentArrayTransformer.forward :221, :230-232, fused with the EDM coefficients :424-429; norm.hip),
 * fp32 throughout.  coef[s][coef_stride] = {c_in, c_skip, c_out, ...} of the sample s = row / rows_per_group.
 *   proj_in:         x[m][n] = c_in * sum_k xin[m][k] W[n][k]                                   W [D][C]
 *   final_norm_proj: out[m][c] = c_skip * xin[m][c] + c_out * sum_k LN(x[m]; gamma, beta)[k] Wout[c][k]     Wout [C][D], D = 512 */
int rald_op_proj_in(const float* xin, const float* W, float* x, int32_t M, int32_t C, int32_t D, const float* coef, int32_t coef_stride,
                    int32_t rows_per_group, void* stream);
int rald_op_final_norm_proj(const float* x, const float* gamma, const float* beta, const float* Wout, const float* xin, float* out, int32_t M,
                            int32_t D, int32_t C, const float* coef, int32_t coef_stride, int32_t rows_per_group, void* stream);
int rald_op_reduce_resid_ln(const float* part, int32_t slabs, int64_t slab_stride, const float* bias, float* x, void* h_bf16, int32_t M,
                            const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps, void* stream);
/* Streaming query decoder (KLAutoEncoder.decode :417-424; rald_amd/csrc/ae_decode.hip).  _tables: the weight-only tables
 * it is built on, computed on the HOST in double from host tensors of decoder_cross_attn (to_q [d,d], k half of to_kv [d,d],
 * norm weight / bias [d]), point_embed.mlp (weight [d,51], bias [d]) and the folded value vector [d]:
 * t2aug_out [d][64] fp32, l_img_out [64][64] fp16 bits (no GPU needed: what the CPU tests check the folding with). */
int rald_op_ae_decode_tables(int32_t dim, const float* wq, const float* wk, const float* norm_w, const float* norm_b, const float* wpe,
                             const float* bpe, const float* wfold, float* t2aug_out, uint16_t* l_img_out);
/* rald_op_ae_decode: the decoder on such tables, as rald_ae_decode_latents ends and rald_ae_decode_queries runs it.  All device memory:
 * x fp32 [batch*num_latents][dim] (output of the latent stack), gamma / beta [dim] (norm_context), t2aug [dim][64], l_img [64][64] fp16
 * (16-byte aligned), basis [3][24] (block-diagonal -> one multiply per projection, anything else -> three; decided here as at weight load),
 * queries fp32 [batch][n_queries][3] -> out_logits fp32 [batch][n_queries].  dim 256 or 512, num_latents a multiple of 32 in [32,1024],
 * batch in [1,65535]; scratch (16-byte aligned) of rald_op_ae_decode_scratch_bytes(batch, num_latents) bytes (-1: refused). */
int64_t rald_op_ae_decode_scratch_bytes(int32_t batch, int32_t num_latents);
int rald_op_ae_decode(const float* x, const float* gamma, const float* beta, const float* t2aug, const uint16_t* l_img, const float* basis,
                      float c0, const float* queries, float* out_logits, int32_t batch, int64_t n_queries, int32_t num_latents, int32_t dim,
                      void* scratch, int64_t scratch_bytes, void* stream);
/* rald_op_ae_cast_rays: rald_ae_cast_rays on caller-made tables, with rald_op_ae_decode's arguments, checks and scratch. */
int rald_op_ae_cast_rays(const float* x, const float* gamma, const float* beta, const float* t2aug, const uint16_t* l_img, const float* basis,
                         float c0, const float* origins, const float* dirs, int64_t ray_batch_stride, int32_t n_steps, int32_t n_refine,
                         float* out_t, float* out_logit, int32_t* out_step, float* out_points, int32_t batch, int64_t n_rays,
                         int32_t num_latents, int32_t dim, void* scratch, int64_t scratch_bytes, void* stream);
/* rald_op_ae_decode_grad: rald_op_ae_decode's arguments and checks (num_latents <= 512 here) + offsets (NULL: dense; else DEVICE int64
 * [batch+1], queries / outputs concatenated and n_queries = the host bound of the longest segment), out_grad, out_projected (NULL to
 * skip) and max_step as rald_ae_decode_queries_grad.  Same scratch as rald_op_ae_decode. */
int rald_op_ae_decode_grad(const float* x, const float* gamma, const float* beta, const float* t2aug, const uint16_t* l_img, const float* basis,
                           float c0, const float* queries, const int64_t* offsets, float* out_logits, float* out_grad, float* out_projected,
                           float max_step, int32_t batch, int64_t n_queries, int32_t num_latents, int32_t dim, void* scratch,
                           int64_t scratch_bytes, void* stream);
/* Folded encoder (KLAutoEncoder.encode :351-399; rald_amd/csrc/ae_encode.hip): both attentions of the latent queries over the
 * input points run with ONE fp16 row of 52 Fourier features per point as key and value (head dim 64).
 * _tables: the weight-only tables, computed on the HOST in double (no GPU needed).  in[18] = host fp32 tensors in the reference's
 *   layouts: point_embed.mlp weight [d,51], bias [d]; d_latents [M,d]; mix_attn_layer norm weight, bias [d], to_q [I,d], to_kv [2I,d],
 *   to_out weight [d,I], bias [d]; s_latents (mix) or latents (learnable) [M,d]; query_proj weight [d,d], bias [d];
 *   cross_attend_blocks.0 norm_context weight, bias [d], to_q [d,d], to_kv [2d,d], to_out weight [d,d], bias [d]   (I = heads*64; entries
 *   2-8, 10, 11 may be null when mix == 0).  out[7] (any may be null) = variance factor [52,52], mix queries [M,I], T4 [d,I], X0 [M,d],
 *   T1 [d,64], T3 [d,64], c3 [d] - see ae_encode.hip for what each multiplies.
 * _features: F, G fp16 [batch][rows_per_sample][64] from pc [batch][n_points][3] (rows_per_sample = n_points rounded up to 64).
 * rald_op_attention_f16kv: the attention kernel's fp16 form on such rows (rows nk .. k_rows-1 must be ZERO, as _features writes them; fp32
 *   queries already times scale*log2(e); ksplit < 0 = pick;
 *   scratch = rald_op_attention_split_scratch_bytes(16, ...) when the keys may be split).
 * _qproj: the step between the two attentions.  x [rows][dim] = (xin ? xin : 0) + X0[row % num_latents] (fp32, kept; xin may be x itself)
 *   and Q [rows][64] fp32 = LayerNorm(x; gamma, beta) . T1 [dim][64]; dim 256 or 512, xin may be NULL ('learnable': x = the latents). */
int rald_op_ae_encode_tables(int32_t dim, int32_t num_latents, int32_t heads, int32_t mix, const float* const* in, float* const* out);
int rald_op_ae_enc_features(const float* pc, const float* basis, const float* var_factor, void* F_f16, void* G_f16, int32_t batch, int32_t n_points,
                            int32_t rows_per_sample, void* stream);
int rald_op_ae_enc_qproj(const float* xin, const float* X0, float* x, const float* gamma, const float* beta, const float* T1, float* Q,
                         int32_t rows, int32_t num_latents, int32_t dim, void* stream);
int rald_op_attention_f16kv(const float* Q, int64_t ldq, int64_t strideQ, const void* KV_f16, void* O_bf16, int64_t ldo, int64_t strideO, int32_t nq,
                            int32_t nk, int32_t k_rows, int32_t heads, int32_t batch, int32_t ksplit, void* scratch, void* stream);
/* MXFP8 (OCP microscaling: e4m3 elements + one e8m0 scale per 32 consecutive K elements of a row), the
 * "fp8 MFMA QKV/proj path" of BASELINE config #5.  C = alpha * A . B^T + bias on
 * v_mfma_scale_f32_16x16x128_f8f6f4; epilogue 0 = bf16, 1 = f32, 2 = f32 residual accumulate.  K % 128 == 0;
 * lda/ldb/strides in bytes (= elements); scales [rows][K/32] contiguous per batch entry.  alpha applies to the output columns
 * n < alpha_ncols (a multiple of 4; 1 << 30 = all of them), the others use 1. */
int rald_op_gemm_mx8(const void* A8, const void* scaleA, int64_t lda, int64_t strideA, int64_t strideSA, const void* B8, const void* scaleB,
                     int64_t ldb, int64_t strideB, int64_t strideSB, void* C, int64_t ldc, int64_t strideC, const float* bias, int32_t M,
                     int32_t N, int32_t K, int32_t batch, float alpha, int32_t epilogue, void* stream, int32_t alpha_ncols);
/* the tile rald_op_gemm_mx8 runs such a problem on, by the dispatcher's own rule: 256 (256 x 256 tiles) or 128 */
int rald_op_gemm_mx8_tile(int32_t M, int32_t N, int32_t batch);
/* rows of f32 (in_is_bf16 = 0) or bf16 -> MXFP8: block scale = the smallest power of two with amax / scale <= 448 */
int rald_op_quantize_mx8(const void* in, int32_t in_is_bf16, int64_t ld_in, void* out_e4m3, int64_t ld_out, void* out_scales_e8m0, int64_t rows,
                         int32_t K, void* stream);
/* rald_op_layernorm with an MXFP8 result (D = 512) */
int rald_op_layernorm_mx8(const float* x, void* out_e4m3, void* out_scales_e8m0, int64_t M, int32_t D, const float* g, const float* b,
                          int64_t gstride, int32_t rows_per_group, float add_one, float eps, void* stream);
/* out_bf16 = LayerNorm(x_f32[M][D]) * (add_one + g[row/rows_per_group*gstride + c]) + b[...] */
int rald_op_layernorm(const float* x, void* out_bf16, int32_t M, int32_t D, const float* g, const float* b,
                      int64_t gstride, int32_t rows_per_group, float add_one, float eps, void* stream);
/* multi-head attention, head dim 64; Q[b][i][h*64+d], K[b][j][h*64+d], Vt[b][h*64+d][j] bf16.  q_prescaled != 0: Q is already
 * multiplied by scale*log2(e) (as the denoiser's projections produce it) and `scale` is ignored. */
int rald_op_attention(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                      const void* Vt, int64_t ldvt, int64_t strideVt, void* O, int64_t ldo, int64_t strideO,
                      int32_t nq, int32_t nk, int32_t k_rows, int32_t heads, int32_t batch, float scale, int32_t q_prescaled, void* stream);
/* rald_op_attention with the keys split over `ksplit` workgroups per query block (few queries x many keys, e.g. 512
 * latents x 10 000 points at batch 1): partial results go through `scratch` (rald_op_attention_split_scratch_bytes)
 * and a combine pass.  ksplit <= 0 picks a value from the shape. */
int64_t rald_op_attention_split_scratch_bytes(int32_t ksplit, int32_t nq, int32_t heads, int32_t batch);
int rald_op_attention_split(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, const void* Vt, int64_t ldvt,
                            int64_t strideVt, void* O, int64_t ldo, int64_t strideO, int32_t nq, int32_t nk, int32_t k_rows, int32_t heads,
                            int32_t batch, float scale, int32_t ksplit, void* scratch, void* stream);
/* rald_op_attention with V row-major like K (V[b][j][h*64+d], e.g. a column slice of a fused q|k|v projection): the kernel
 * transposes it on the LDS read (ds_read_b64_tr_b16).  nk % 64 == 0 (rald_op_attention_args takes a ragged nk with a zero pad). */
int rald_op_attention_vrow(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, const void* V, int64_t ldv,
                           int64_t strideV, void* O, int64_t ldo, int64_t strideO, int32_t nq, int32_t nk, int32_t heads, int32_t batch, float scale,
                           void* stream);
/* The attention kernel with every field of its argument block from the caller (tests; the entries above fix some of them).
 *   queries   Q_bf16 [b][i][h*64+d], or Qf fp32 with f16 != 0 (the fp16 form: K and V hold fp16, q_prescaled and a row-major V required);
 *             strideQ = 0 shares one set of queries between the batch entries
 *   keys      K [b][j][h*hsk+d], hsk = 64, or 0 = every head reads the same 64 columns (of K and of V / Vt); k_rows >= nk rounded up to
 *             64 rows are allocated per batch entry and read; rows nk.. may hold any finite values (they are masked)
 *   values    Vt [b][h*hsk+d][j] with ldvt >= nk rounded up to 64, columns nk.. any finite values; or V [b][j][h*hsk+d] row-major with
 *             nk % 64 == 0, or with v_padded != 0 and rows nk .. k_rows-1 ZERO (the pad contract of the row-major and fp16 forms)
 *   output    O_bf16 [b][i][h*64+d]; only columns h*64 .. h*64+63 of rows 0 .. nq-1 are written (ldo may be wider)
 *   q_prescaled != 0: the queries already carry scale*log2(e) and `scale` is ignored
 *   ksplit    0 / 1 = one pass; 2..64 = that many key ranges per query block + the combine pass; < 0 = pick from the shape;
 *             scratch (8-byte aligned) of rald_op_attention_split_scratch_bytes(ksplit, nq, heads, batch) bytes when the keys are split
 * nq % 32 == 0; leading dimensions multiples of 8 elements; 16-byte aligned pointers. */
int rald_op_attention_args(const void* Q_bf16, const float* Qf, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                           int32_t k_rows, const void* Vt, int64_t ldvt, int64_t strideVt, const void* V, int64_t ldv, int64_t strideV, void* O_bf16,
                           int64_t ldo, int64_t strideO, int32_t nq, int32_t nk, int32_t heads, int32_t batch, float scale, int32_t q_prescaled,
                           int32_t f16, int32_t hsk, int32_t v_padded, int32_t ksplit, void* scratch, int64_t scratch_bytes, void* stream);
int32_t rald_op_attention_pick_ksplit(int32_t nq, int32_t nk, int32_t heads, int32_t batch);
/* gradients of rald_op_attention_vrow's O = softmax(Q K^T scale) V per head (torch autograd of CrossAttention,
 * model/models_radar_generation.py:66-75, in the training step engine_generation.py:74-98): dQ, dK, dV bf16 in the layouts of Q, K, V
 * (own leading dimensions and batch strides: column slices of fused buffers are fine).  Two launches, nothing score-shaped in memory.
 * lse_scratch / delta_scratch: fp32 [batch*heads*nq] each.  nq % 128 == 0; nk any >= 32 (a last key tile that is not full is masked:
 * nothing past key nk - 1 is read or written). */
int rald_op_attention_bwd(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, const void* V, int64_t ldv,
                          int64_t strideV, const void* O, int64_t ldo, int64_t strideO, const void* dO, int64_t lddo, int64_t strideDO,
                          void* dQ, int64_t lddq, int64_t strideDQ, void* dK, int64_t lddk, int64_t strideDK, void* dV, int64_t lddv, int64_t strideDV,
                          float* lse_scratch, float* delta_scratch, int32_t nq, int32_t nk, int32_t heads, int32_t batch, float scale, void* stream);
/* fused residual GEMM + next LayerNorm (N = 512): x[M][512] += A[M][K].W[512][K]^T + bias (fp32, in place);
 * h_bf16 = LayerNorm(x) * (add_one + g[row/rows_per_group*gstride + c]) + b[...] */
int rald_op_gemm_resid_ln(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* x, void* h_bf16,
                          const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps,
                          int32_t M, int32_t K, void* stream);
/* The residual projection as the latent stacks run it, with every field of its argument block reachable (tests): bf16 operands
 * (A_bf16, W_bf16) or MXFP8 ones (A8 / SA, W8 / SW: e4m3 + e8m0 scales [..][K/32]; the other form's pointers null); h_bf16 or the
 * MXFP8 form h8 [M][512] / hs [M][16]; g / b null = no LayerNorm (route 0 only); strideW != 0: rows [i*w_rows, (i+1)*w_rows)
 * multiply W + i*strideW; nt_io: non-temporal residual / output traffic of the fused kernel.
 * route 0 = the dispatcher the models call (split-K slabs through `scratch` + reduction, the fused kernel, or GEMM + LayerNorm, by M and K);
 * route 1 = the fused kernel directly.  scratch: at least 4 * M * 512 * 4 bytes when route 0 splits K (K >= 2048 and M <= 4096). */
int rald_op_resid_gemm_ln(const void* A_bf16, const void* A8, const void* SA, int64_t lda, const void* W_bf16, const void* W8, const void* SW,
                          int64_t ldw, int64_t strideW, int32_t w_rows, const float* bias, float* x, void* h_bf16, void* h8, void* hs,
                          const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps, int32_t M,
                          int32_t K, int32_t nt_io, int32_t route, void* scratch, int64_t scratch_bytes, void* stream);
/* The GEGLU projection (packed W rows and bias, as epilogue 3 of rald_op_gemm_nt) on bf16 or MXFP8 operands, into out_bf16 [M][ldc] or
 * into the MXFP8 form out8 [M][ldc] / outs [M][N/64] that the MXFP8 residual GEMM reads (full 256x256 tiles only). */
int rald_op_gemm_geglu_mx8out(const void* A_bf16, const void* A8, const void* SA, int64_t lda, const void* W_bf16, const void* W8, const void* SW,
                              int64_t ldw, const float* bias_packed, void* out_bf16, void* out8, void* outs, int64_t ldc, int32_t M, int32_t N,
                              int32_t K, void* stream);
int rald_op_cast_bf16(const float* in, void* out_bf16, int64_t n, void* stream);
/* Set-latent autoencoder training (KLAutoEncoder under autograd, engine_ae.py:33-104; rald_amd/csrc/ae_train.hip).  No float atomics:
 * reductions over rows go through a caller-owned scratch (16-byte aligned, _scratch_bytes(rows) bytes - pure host arithmetic) and are
 * summed in a fixed order by a second launch, so results are bit-reproducible.
 * _ln_affine_bwd: nn.LayerNorm(512) backward, x [rows][512] fp32 (the LN input), dh [rows][512] fp32 (gradient w.r.t. the LN output):
 *   dx_accum += dx; dx_bf16_out (nullable) = the updated dx_accum as bf16; dgamma_accum / dbeta_accum [512] += sum dh*xhat / sum dh.
 * _pe_wgrad: PointEmbed.mlp gradient from dY [rows][512] fp32 and the raw points [rows][3] (basis [3][24]): dW_accum [512][51] +=
 *   dY^T . [sin(p.basis) | cos(p.basis) | p], db_accum [512] += column sums of dY.
 * _point_features: feat bf16 [n][64] = [sin(p.basis) (24) | cos (24) | p (3) | 0 ...].
 * _posterior: ml [B*rows][2L] = raw [mean | logvar] -> z [B*rows][L] = mean + exp(0.5 clamp(logvar, -30, 20)) eps, kl [B].
 * _posterior_bwd: dml [B*rows][2L] = gradient of (z, kl) w.r.t. [mean | logvar] given dz (nullable) and dkl [B] (nullable).
 * _scale_rows: drop-path residual; exactly one of x_accum (x += s[r / rows_per_sample] * in[r]) and out_bf16 (= s[...] * in[r]).
 * _softmax_bwd_rows: S [rows][ld] fp32 (already times the softmax scale), dP [rows][ld], delta [rows]: P = softmax of S[r][0..n),
 *   dS = P (dP - delta[r]) * scale; P (nullable) and dS bf16 [rows][ld], columns n .. ld - 1 zero. */
int64_t rald_op_ln_affine_bwd_scratch_bytes(int64_t rows);
int rald_op_ln_affine_bwd(const float* x, const float* dh, const float* gamma, float eps, int64_t rows, float* dx_accum, void* dx_bf16_out,
                          float* dgamma_accum, float* dbeta_accum, void* scratch, int64_t scratch_bytes, void* stream);
int64_t rald_op_pe_wgrad_scratch_bytes(int64_t rows);
int rald_op_pe_wgrad(const float* dY, const float* pts, const float* basis, int64_t rows, float* dW_accum, float* db_accum, void* scratch,
                     int64_t scratch_bytes, void* stream);
int rald_op_point_features(const float* pts, const float* basis, void* feat_bf16, int64_t n, void* stream);
int rald_op_posterior(const float* ml, const float* eps, float* z, float* kl, int32_t B, int32_t rows, int32_t L, void* stream);
int rald_op_posterior_bwd(const float* dz, const float* dkl, const float* ml, const float* eps, float* dml, int32_t B, int32_t rows, int32_t L,
                          void* stream);
int rald_op_scale_rows(const float* in, const float* s, float* x_accum, void* out_bf16, int64_t rows, int32_t cols, int64_t rows_per_sample,
                       void* stream);
int rald_op_softmax_bwd_rows(const float* S, const float* dP, const float* delta, int64_t rows, int64_t ld, int32_t n, float scale, void* P_bf16,
                             void* dS_bf16, void* stream);
/* The stage-1 loss, its metrics and its gradient (engine_ae.py:70-101) for logits / labels [batch][n_queries] fp32 (labels exactly 0 or 1)
 * and kl [batch].  n = *in_voxel_num_dev (device int32, clamped to [0, n_queries]) is read by the kernels, so a captured graph serves any
 * split point.  out_losses4 (device double[4]) = [vol_weight vol + near_weight near + kl_weight kl, vol, near, kl]: vol / near = the mean of
 * max(x, 0) - x y + log1p(exp(-|x|)) over [:, :n] / [:, n:] (NaN for an empty span, as torch's mean), kl = sum(kl) / batch; the total is not
 * multiplied by grad_scale.  out_counts3 (device int32 [batch][3]) = (#(pred == label), #(pred and label), #(pred or label)) with
 * pred = (x >= 0).  dlogits [batch][n_queries] (nullable) = grad_scale * w_span / (batch * n_span) * (sigmoid(x) - y); dkl [batch]
 * (nullable) = grad_scale * kl_weight / batch.  Sums are accumulated in double through per-workgroup partials in the caller-owned scratch
 * (16-byte aligned, _scratch_bytes(batch, n_queries) bytes - host arithmetic) and added in a fixed order: no float atomics, the same bits
 * run to run, and one sample's counts and dlogits row do not depend on the rest of the batch.  Two launches. */
int64_t rald_op_ae_loss_scratch_bytes(int32_t batch, int64_t n_queries);
int rald_op_ae_loss(const float* logits, const float* labels, const float* kl, const int32_t* in_voxel_num_dev, int32_t batch, int64_t n_queries,
                    float vol_weight, float near_weight, float kl_weight, float grad_scale, double* out_losses4, int32_t* out_counts3,
                    float* dlogits, float* dkl, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RALD_HIP_H */
