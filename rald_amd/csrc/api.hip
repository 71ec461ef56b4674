// extern "C" surface of librald_hip.so (include/rald_hip.h).  Thin: argument checks + dispatch.
#include <cstdlib>
#include <cstring>

#include "ae.h"
#include "cloud_index.h"
#include "dit.h"
#include "lidar.h"
#include "radar_dsp.h"
#include "radar_points.h"

using namespace rald;

struct rald_dit { Dit impl; };
struct rald_ae { Ae impl; };

extern "C" {

const char* rald_last_error(void) { return rald::last_error(); }
int rald_version(void) { return 3; }
int rald_build_flags(void) { return 0; }

int64_t rald_debug_f16_saturation_count(int32_t reset) {
    unsigned a = 0, b = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (f16_saturation_gemm(&a, reset != 0) || f16_saturation_attn(&b, reset != 0)) return -1;
    return (int64_t)a + (int64_t)b;
}

// the per-head slabs of attn_self_proj / xattn_q2_proj alone
int64_t rald_debug_f16_saturation_attn(int32_t reset) {
    unsigned a = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (f16_saturation_attn(&a, reset != 0)) return -1;
    return (int64_t)a;
}

int rald_debug_poison_lds(void* stream) { return poison_lds((hipStream_t)stream); }

void rald_dit_default_config(rald_dit_config* c) {
    c->n_latents = 512; c->channels = 32; c->depth = 24; c->n_heads = 8; c->d_head = 64; c->t_channels = 256;
    c->context_dim = 512; c->n_cond_tokens = 64; c->with_radar_enc = 1; c->enc_hidden_ch = 64; c->enc_radar_ch = 16;
    c->radar_r = 128; c->radar_a = 64; c->radar_e = 32; c->sigma_data = 1.0f; c->qkv_dtype = 0;
}
int rald_dit_create(const rald_dit_config* cfg, rald_dit** out) {
    RALD_CHECK(cfg && out, "rald_dit_create: null argument");
    rald_dit* h = new rald_dit();
    h->impl.cfg = *cfg;
    int rc = h->impl.create();
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}
void rald_dit_destroy(rald_dit* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h;
}
int rald_dit_load_weight(rald_dit* h, const char* name, const float* data, int64_t nelem) {
    RALD_CHECK(h && name && data, "rald_dit_load_weight: null argument");
    return h->impl.load_weight(name, data, nelem);
}
int rald_dit_finalize(rald_dit* h) { RALD_CHECK(h, "null handle"); return h->impl.finalize(); }
int rald_dit_reserve(rald_dit* h, int32_t max_batch) {
    RALD_CHECK(h && max_batch >= 1, "rald_dit_reserve: bad argument");
    return h->impl.reserve(max_batch);
}
int64_t rald_dit_workspace_generation(const rald_dit* h) { return h ? h->impl.ws_generation : -1; }
int rald_dit_set_two_stream_min_batch(rald_dit* h, int32_t min_batch) {
    RALD_CHECK(h && min_batch >= 0, "rald_dit_set_two_stream_min_batch: bad argument");
    h->impl.split_min = min_batch;
    if (h->impl.ws_batch > 0) {                  // re-plan the workspace (the second half's buffers exist only when the split can happen)
        const int B = h->impl.ws_batch;
        h->impl.ws_batch = 0;
        return h->impl.reserve(B);
    }
    return 0;
}
int32_t rald_dit_two_stream_min_batch(const rald_dit* h) { return h ? h->impl.split_min : -1; }
int rald_dit_set_sigmas(rald_dit* h, const float* sigmas_host, int32_t n, void* stream) {
    RALD_CHECK(h && sigmas_host, "rald_dit_set_sigmas: null argument");
    return h->impl.set_sigmas(sigmas_host, n, (hipStream_t)stream);
}
int64_t rald_dit_cond_cache_bytes(const rald_dit* h, int32_t batch) { return h ? h->impl.cond_cache_bytes(batch) : -1; }
int rald_dit_encode_cond_tokens(rald_dit* h, const float* tokens, int32_t batch, void* cond_cache, void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.encode_cond_tokens(tokens, batch, cond_cache, (hipStream_t)stream);
}
int rald_dit_encode_cond(rald_dit* h, const float* cube, int32_t batch, float* out_tokens, void* cond_cache, void* stream) {
    RALD_CHECK(h && cube && cond_cache && batch >= 1, "rald_dit_encode_cond: bad argument");
    return h->impl.encode_cond(cube, batch, out_tokens, cond_cache, (hipStream_t)stream);
}
int rald_dit_denoise(rald_dit* h, const float* x, int32_t batch, int32_t sigma_row, int32_t per_sample,
                     const void* cond_cache, float* out, int32_t raw_F, void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.denoise(x, batch, sigma_row, per_sample, cond_cache, out, raw_F, (hipStream_t)stream);
}
int rald_dit_sample(rald_dit* h, const float* latents, int32_t batch, const void* cond_cache, int32_t num_steps,
                    float sigma_min, float sigma_max, float rho, float* out, void* stream) {
    RALD_CHECK(h && latents && cond_cache && out && batch >= 1, "rald_dit_sample: bad argument");
    return h->impl.sample(latents, batch, cond_cache, num_steps, sigma_min, sigma_max, rho, out, (hipStream_t)stream);
}
int rald_edm_schedule(int32_t num_steps, double sigma_min, double sigma_max, double rho, double S_churn, double S_min, double S_max, float* t,
                      float* t_hat) {
    return edm_schedule(num_steps, sigma_min, sigma_max, rho, S_churn, S_min, S_max, t, t_hat);
}
int rald_dit_sample_stochastic(rald_dit* h, const float* latents, int32_t batch, const void* cond_cache, int32_t num_steps, double sigma_min,
                               double sigma_max, double rho, double S_churn, double S_min, double S_max, double S_noise, const float* noise,
                               const int64_t* seeds, float* out, void* stream) {
    RALD_CHECK(h && latents && cond_cache && out && batch >= 1, "rald_dit_sample_stochastic: bad argument");
    return h->impl.sample_stochastic(latents, batch, cond_cache, num_steps, sigma_min, sigma_max, rho, S_churn, S_min, S_max, S_noise, noise,
                                     seeds, out, (hipStream_t)stream);
}
int rald_op_philox_normal(const int64_t* seeds, int32_t B, int64_t n_per_sample, int32_t tag, int32_t step, float* out, void* stream) {
    return philox_normal(seeds, B, n_per_sample, tag, step, out, (hipStream_t)stream);
}

int rald_dit_profile_begin(rald_dit* h) { RALD_CHECK(h, "null handle"); h->impl.prof_mask = 0xf; return h->impl.profile_begin(); }
int rald_dit_profile_set_kinds(rald_dit* h, uint32_t kind_mask) {
    RALD_CHECK(h, "null handle");
    h->impl.prof_mask = kind_mask & 0xfu;
    return 0;
}
int rald_dit_profile_end(rald_dit* h, double* total_ms, int32_t* launches) {
    RALD_CHECK(h && total_ms && launches, "rald_dit_profile_end: null argument");
    int n = 0;
    int rc = h->impl.profile_end(total_ms, &n);
    *launches = n;
    return rc;
}

int rald_dit_profile_end_kinds(rald_dit* h, double* total_ms4, int32_t* launches4) {
    RALD_CHECK(h && total_ms4 && launches4, "rald_dit_profile_end_kinds: null argument");
    int n[Dit::PROF_KINDS];
    int rc = h->impl.profile_end_kinds(total_ms4, n);
    for (int k = 0; k < Dit::PROF_KINDS; ++k) launches4[k] = n[k];
    return rc;
}

// ---- autoencoder ---------------------------------------------------------------------------------
int rald_ae_create(const rald_ae_config* cfg, rald_ae** out) {
    RALD_CHECK(cfg && out, "rald_ae_create: null argument");
    rald_ae* h = new rald_ae();
    h->impl.cfg = *cfg;
    int rc = h->impl.create();
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}
void rald_ae_destroy(rald_ae* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h;
}
int rald_ae_load_weight(rald_ae* h, const char* name, const float* data, int64_t nelem) {
    RALD_CHECK(h && name && data, "rald_ae_load_weight: null argument");
    return h->impl.load_weight(name, data, nelem);
}
int rald_ae_finalize(rald_ae* h) { RALD_CHECK(h, "null handle"); return h->impl.finalize(); }
int rald_ae_encode(rald_ae* h, const float* pc, int32_t batch, const float* eps, float* out_mean, float* out_logvar,
                   float* out_z, float* out_kl, void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.encode(pc, batch, eps, out_mean, out_logvar, out_z, out_kl, (hipStream_t)stream);
}
int64_t rald_ae_ctx_bytes(const rald_ae* h, int32_t batch) { return h ? h->impl.ctx_bytes(batch) : -1; }
int64_t rald_ae_workspace_generation(const rald_ae* h) { return h ? h->impl.ws_generation : -1; }
int rald_ae_decode_latents(rald_ae* h, const float* z, int32_t batch, void* ctx, void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.decode_latents(z, batch, ctx, (hipStream_t)stream);
}
int rald_ae_decode_queries(rald_ae* h, const void* ctx, const float* queries, int32_t batch, int64_t n_queries,
                           float* out_logits, void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.decode_queries(ctx, queries, batch, n_queries, out_logits, (hipStream_t)stream);
}
int rald_ae_decode_queries_ragged(rald_ae* h, const void* ctx, const float* queries, const int64_t* offsets, int32_t batch,
                                  int64_t max_per_sample, float* out_logits, void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.decode_queries_ragged(ctx, queries, offsets, batch, max_per_sample, out_logits, (hipStream_t)stream);
}
int rald_ae_decode_queries_grad(rald_ae* h, const void* ctx, const float* queries, int32_t batch, int64_t n_queries, float* out_logits,
                                float* out_grad, float* out_projected, float max_step, void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.decode_queries_grad(ctx, queries, nullptr, batch, n_queries, out_logits, out_grad, out_projected, max_step, (hipStream_t)stream);
}
int rald_ae_decode_queries_grad_ragged(rald_ae* h, const void* ctx, const float* queries, const int64_t* offsets, int32_t batch,
                                       int64_t max_per_sample, float* out_logits, float* out_grad, float* out_projected, float max_step,
                                       void* stream) {
    RALD_CHECK(h, "null handle");
    RALD_CHECK(offsets, "rald_ae_decode_queries_grad_ragged: null offsets");
    return h->impl.decode_queries_grad(ctx, queries, offsets, batch, max_per_sample, out_logits, out_grad, out_projected, max_step,
                                       (hipStream_t)stream);
}
int rald_ae_cast_rays(rald_ae* h, const void* ctx, const float* origins, const float* dirs, int64_t ray_batch_stride, int32_t batch,
                      int64_t n_rays, int32_t n_steps, int32_t n_refine, float* out_t, float* out_logit, int32_t* out_step, float* out_points,
                      void* stream) {
    RALD_CHECK(h, "null handle");
    return h->impl.cast_rays(ctx, origins, dirs, ray_batch_stride, batch, n_rays, n_steps, n_refine, out_t, out_logit, out_step, out_points,
                             (hipStream_t)stream);
}

// test entry point of the streaming query decoder (ae_decode.hip)
int rald_op_ae_decode_tables(int32_t dim, const float* wq, const float* wk, const float* norm_w, const float* norm_b, const float* wpe,
                             const float* bpe, const float* wfold, float* t2aug_out, uint16_t* l_img_out) {
    RALD_CHECK(wq && wk && norm_w && norm_b && wpe && bpe && wfold && t2aug_out && l_img_out && dim >= 64, "rald_op_ae_decode_tables: bad argument");
    std::vector<float> t2;
    std::vector<unsigned short> li;
    RALD_TRY(rald::ae_decode_tables(dim, wq, wk, norm_w, norm_b, wpe, bpe, wfold, t2, li));
    memcpy(t2aug_out, t2.data(), t2.size() * 4);
    memcpy(l_img_out, li.data(), li.size() * 2);
    return 0;
}
// the decoder itself on caller-made tables: the context build and the streaming kernel of Ae::decode_latents / Ae::decode_queries, the
// kernel's form picked from the basis by the same rule.  Every argument check comes before the first HIP call.
int64_t rald_op_ae_decode_scratch_bytes(int32_t batch, int32_t num_latents) {
    if (batch < 1 || batch > 65535 || num_latents < 32 || num_latents > 1024 || num_latents % 32) return -1;
    return ae_decode_op_scratch_bytes(batch, num_latents);
}
int rald_op_ae_decode(const float* x, const float* gamma, const float* beta, const float* t2aug, const uint16_t* l_img, const float* basis,
                      float c0, const float* queries, float* out_logits, int32_t batch, int64_t n_queries, int32_t num_latents, int32_t dim,
                      void* scratch, int64_t scratch_bytes, void* stream) {
    RALD_CHECK(x && gamma && beta && t2aug && l_img && basis && queries && out_logits && scratch, "rald_op_ae_decode: null pointer");
    RALD_CHECK(dim == 256 || dim == 512, "rald_op_ae_decode: dim must be 256 or 512");
    RALD_CHECK(num_latents >= 32 && num_latents <= 1024 && num_latents % 32 == 0,
               "rald_op_ae_decode: num_latents must be a multiple of 32 in [32,1024]");
    RALD_CHECK(batch >= 1 && batch <= 65535, "rald_op_ae_decode: batch must be in [1,65535]");
    RALD_CHECK(n_queries >= 1, "rald_op_ae_decode: n_queries must be at least 1");
    RALD_CHECK((uintptr_t)scratch % 16 == 0 && (uintptr_t)l_img % 16 == 0, "rald_op_ae_decode: scratch and l_img must be 16-byte aligned");
    RALD_CHECK(scratch_bytes >= ae_decode_op_scratch_bytes(batch, num_latents), "rald_op_ae_decode: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    float h_basis[72];
    RALD_HIP(hipMemcpyAsync(h_basis, basis, sizeof(h_basis), hipMemcpyDeviceToHost, st));
    RALD_HIP(hipStreamSynchronize(st));
    void* ctx = (char*)scratch + ae_decode_op_ctx_offset(batch, num_latents);
    RALD_TRY(ae_ctx_build(x, gamma, beta, t2aug, (float*)scratch, ctx, batch, num_latents, dim, st));
    return ae_decode_stream(ctx, l_img, queries, out_logits, basis, ae_basis_is_block_diagonal(h_basis), batch, n_queries, num_latents, c0, st);
}
// the gradient decoder on caller-made tables: rald_op_ae_decode's checks, then the same context build and ae_decode_grad_stream.  offsets
// NULL: dense, n_queries per sample; else the ragged layout of rald_ae_decode_queries_ragged with n_queries = max_per_sample.
int rald_op_ae_decode_grad(const float* x, const float* gamma, const float* beta, const float* t2aug, const uint16_t* l_img, const float* basis,
                           float c0, const float* queries, const int64_t* offsets, float* out_logits, float* out_grad, float* out_projected,
                           float max_step, int32_t batch, int64_t n_queries, int32_t num_latents, int32_t dim, void* scratch,
                           int64_t scratch_bytes, void* stream) {
    RALD_CHECK(x && gamma && beta && t2aug && l_img && basis && queries && out_logits && out_grad && scratch, "rald_op_ae_decode_grad: null pointer");
    RALD_CHECK(dim == 256 || dim == 512, "rald_op_ae_decode_grad: dim must be 256 or 512");
    RALD_CHECK(num_latents >= 32 && num_latents <= AE_DECODE_GRAD_MAX_LATENTS && num_latents % 32 == 0,
               "rald_op_ae_decode_grad: num_latents must be a multiple of 32 in [32,512]");
    RALD_CHECK(batch >= 1 && batch <= 65535, "rald_op_ae_decode_grad: batch must be in [1,65535]");
    RALD_CHECK(n_queries >= 1, "rald_op_ae_decode_grad: n_queries must be at least 1");
    RALD_CHECK(!out_projected || (std::isfinite(max_step) && max_step > 0.f), "rald_op_ae_decode_grad: max_step must be finite and > 0");
    RALD_CHECK((uintptr_t)scratch % 16 == 0 && (uintptr_t)l_img % 16 == 0, "rald_op_ae_decode_grad: scratch and l_img must be 16-byte aligned");
    RALD_CHECK(scratch_bytes >= ae_decode_op_scratch_bytes(batch, num_latents), "rald_op_ae_decode_grad: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    float h_basis[72];
    RALD_HIP(hipMemcpyAsync(h_basis, basis, sizeof(h_basis), hipMemcpyDeviceToHost, st));
    RALD_HIP(hipStreamSynchronize(st));
    void* ctx = (char*)scratch + ae_decode_op_ctx_offset(batch, num_latents);
    RALD_TRY(ae_ctx_build(x, gamma, beta, t2aug, (float*)scratch, ctx, batch, num_latents, dim, st));
    return ae_decode_grad_stream(ctx, l_img, queries, offsets, out_logits, out_grad, out_projected, max_step, basis,
                                 ae_basis_is_block_diagonal(h_basis), batch, n_queries, num_latents, c0, st);
}

// first-return beam casting on caller-made tables: rald_op_ae_decode's checks + the ray checks, all before the first HIP call (a refusal
// leaves every output untouched), then the same context build and ae_cast_rays
int rald_op_ae_cast_rays(const float* x, const float* gamma, const float* beta, const float* t2aug, const uint16_t* l_img, const float* basis,
                         float c0, const float* origins, const float* dirs, int64_t ray_batch_stride, int32_t n_steps, int32_t n_refine,
                         float* out_t, float* out_logit, int32_t* out_step, float* out_points, int32_t batch, int64_t n_rays,
                         int32_t num_latents, int32_t dim, void* scratch, int64_t scratch_bytes, void* stream) {
    RALD_CHECK(x && gamma && beta && t2aug && l_img && basis && origins && dirs && out_t && out_logit && out_step && scratch,
               "rald_op_ae_cast_rays: null pointer");
    RALD_CHECK(dim == 256 || dim == 512, "rald_op_ae_cast_rays: dim must be 256 or 512");
    RALD_CHECK(num_latents >= 32 && num_latents <= 1024 && num_latents % 32 == 0,
               "rald_op_ae_cast_rays: num_latents must be a multiple of 32 in [32,1024]");
    RALD_CHECK(batch >= 1 && batch <= 65535, "rald_op_ae_cast_rays: batch must be in [1,65535]");
    RALD_CHECK(n_rays >= 1 && n_rays <= (1 << 28), "rald_op_ae_cast_rays: n_rays must be in [1,2^28]");
    RALD_CHECK(ray_batch_stride == 0 || ray_batch_stride == 3 * n_rays, "rald_op_ae_cast_rays: ray_batch_stride must be 0 or 3 * n_rays");
    RALD_CHECK(n_steps >= 1 && n_steps <= 65535, "rald_op_ae_cast_rays: n_steps must be in [1,65535]");
    RALD_CHECK(n_refine >= 0 && n_refine <= 30, "rald_op_ae_cast_rays: n_refine must be in [0,30]");
    RALD_CHECK((uintptr_t)scratch % 16 == 0 && (uintptr_t)l_img % 16 == 0, "rald_op_ae_cast_rays: scratch and l_img must be 16-byte aligned");
    RALD_CHECK(scratch_bytes >= ae_decode_op_scratch_bytes(batch, num_latents), "rald_op_ae_cast_rays: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    float h_basis[72];
    RALD_HIP(hipMemcpyAsync(h_basis, basis, sizeof(h_basis), hipMemcpyDeviceToHost, st));
    RALD_HIP(hipStreamSynchronize(st));
    void* ctx = (char*)scratch + ae_decode_op_ctx_offset(batch, num_latents);
    RALD_TRY(ae_ctx_build(x, gamma, beta, t2aug, (float*)scratch, ctx, batch, num_latents, dim, st));
    return ae_cast_rays(ctx, l_img, origins, dirs, ray_batch_stride, basis, ae_basis_is_block_diagonal(h_basis), batch, (int)n_rays, num_latents,
                        n_steps, n_refine, c0, out_t, out_logit, out_step, out_points, st);
}

// ---- standalone radar-spectrum encoder (RadarAutoencoder.encoder) -------------------------------
struct rald_radar { DeviceArena arena; Stager stager; RadarEncoder enc, dec; int R, A, E, cin, zc; bool dec_touched = false; };
int rald_radar_create(int32_t basic_channel, int32_t embed_dim, int32_t in_channels, int32_t R, int32_t A, int32_t E, rald_radar** out) {
    RALD_CHECK(out, "rald_radar_create: null argument");
    rald_radar* h = new rald_radar();
    h->R = R; h->A = A; h->E = E; h->cin = in_channels; h->zc = embed_dim;
    int rc = h->enc.create(basic_channel, embed_dim, R, A, E, 512, &h->arena, in_channels);
    if (!rc) rc = h->dec.create_decoder(basic_channel, embed_dim, 2, R, A, E, &h->arena);
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}
void rald_radar_destroy(rald_radar* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h;
}
int rald_radar_load_weight(rald_radar* h, const char* name, const float* data, int64_t nelem) {
    RALD_CHECK(h && name && data, "rald_radar_load_weight: null argument");
    return h->enc.load_weight(name, data, nelem, h->stager);
}
int rald_radar_load_decoder_weight(rald_radar* h, const char* name, const float* data, int64_t nelem) {
    RALD_CHECK(h && name && data, "rald_radar_load_decoder_weight: null argument");
    h->dec_touched = true;
    return h->dec.load_weight(name, data, nelem, h->stager);
}
int rald_radar_finalize(rald_radar* h) {
    RALD_CHECK(h, "null handle");
    std::string missing;
    RALD_CHECK(h->enc.all_loaded(&missing), "radar encoder: missing key '" + missing + "' (strict load)");
    // the decoder is optional (the generation path only encodes); once one of its tensors was loaded, all must be
    RALD_CHECK(!h->dec_touched || h->dec.all_loaded(&missing), "radar decoder: missing key '" + missing + "' (strict load)");
    return 0;
}
int rald_radar_decode(rald_radar* h, const float* z, int32_t batch, float* out_pred4, void* stream) {
    RALD_CHECK(h && z && out_pred4 && batch >= 1, "rald_radar_decode: bad argument");
    std::string missing;
    RALD_CHECK(h->dec.all_loaded(&missing), "radar decoder: weights not loaded ('" + missing + "')");
    return h->dec.decode(z, batch, out_pred4, (hipStream_t)stream);
}
int rald_radar_encode(rald_radar* h, const float* cube, int32_t batch, float* out_z, void* stream) {
    RALD_CHECK(h && cube && out_z && batch >= 1, "rald_radar_encode: bad argument");
    float* z = nullptr;
    RALD_TRY(h->enc.encode(cube, h->cin, batch, &z, (hipStream_t)stream));
    const size_t n = (size_t)batch * (h->R / 16) * (h->A / 16) * (h->E / 16) * h->zc;
    RALD_HIP(hipMemcpyAsync(out_z, z, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---- decode post-processing -----------------------------------------------------
int64_t rald_post_scratch_bytes(int64_t n_queries) { return (int64_t)post_scratch_ints(n_queries) * 4; }
int rald_post_occupied_points(const float* logits, const float* queries, int64_t n_queries, const double* pc_range6_host,
                              int32_t norm_anisotropy, int32_t norm_isotropy, int32_t view_cone_mode, float threshold,
                              float* out_points, int64_t* out_index, int64_t* out_count, void* scratch, void* stream) {
    return post_occupied_points(logits, queries, n_queries, pc_range6_host, norm_anisotropy, norm_isotropy, view_cone_mode, threshold,
                                out_points, out_index, out_count, (int*)scratch, (hipStream_t)stream);
}
int rald_post_occupied_points_ragged(const float* logits, const float* queries, const int64_t* in_offsets, int32_t batch, int64_t n_total,
                                     const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy, int32_t view_cone_mode,
                                     float threshold, float* out_points, int64_t* out_index, int64_t* out_offsets, void* scratch, void* stream) {
    return post_occupied_points_ragged(logits, queries, in_offsets, batch, n_total, pc_range6_host, norm_anisotropy, norm_isotropy,
                                       view_cone_mode, threshold, out_points, out_index, out_offsets, (int*)scratch, (hipStream_t)stream);
}
int rald_post_transform_points(const float* points, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy,
                               int32_t norm_isotropy, int32_t view_cone_mode, float* out_points, void* stream) {
    return post_transform_points(points, n, pc_range6_host, norm_anisotropy, norm_isotropy, view_cone_mode, out_points, (hipStream_t)stream);
}
int rald_post_oriented_points(const float* points, const float* grad, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy,
                              int32_t norm_isotropy, int32_t view_cone_mode, float* out_points, float* out_normals, void* stream) {
    return post_oriented_points(points, grad, n, nullptr, 0, pc_range6_host, norm_anisotropy, norm_isotropy, view_cone_mode, out_points,
                                out_normals, (hipStream_t)stream);
}
int rald_post_oriented_points_ragged(const float* points, const float* grad, const int64_t* offsets, int32_t batch, int64_t n_total,
                                     const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy, int32_t view_cone_mode,
                                     float* out_points, float* out_normals, void* stream) {
    RALD_CHECK(offsets, "rald_post_oriented_points_ragged: null offsets");
    return post_oriented_points(points, grad, n_total, offsets, batch, pc_range6_host, norm_anisotropy, norm_isotropy, view_cone_mode,
                                out_points, out_normals, (hipStream_t)stream);
}
int rald_post_chamfer_sums(const float* pred, int64_t n_pred, const float* gt, int64_t n_gt, double* out_sums2, void* stream) {
    return post_chamfer_sums(pred, n_pred, gt, n_gt, out_sums2, (hipStream_t)stream);
}
int rald_post_chamfer_sums_ragged(const float* pred, const int64_t* pred_offsets, const float* gt, const int64_t* gt_offsets, int32_t batch,
                                  int64_t max_pred, int64_t max_gt, double* out_sums, void* stream) {
    return post_chamfer_sums_ragged(pred, pred_offsets, gt, gt_offsets, batch, max_pred, max_gt, out_sums, (hipStream_t)stream);
}
int rald_post_iou(const float* logits, const float* labels, int32_t batch, int64_t n_queries, float* out_accuracy, float* out_iou, void* stream) {
    return post_iou(logits, labels, batch, n_queries, out_accuracy, out_iou, (hipStream_t)stream);
}

// ---- point-cloud metrics ---------------------------------------------------------
int64_t rald_post_cloud_metrics_scratch_bytes(int32_t batch, int64_t max_pred, int64_t max_gt) {
    return cloud_metrics_scratch_bytes(batch, max_pred, max_gt);
}
int rald_post_nn_ragged(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int32_t batch, int64_t max_a,
                        int64_t max_b, double* out_dist, int64_t* out_idx, void* scratch, void* stream) {
    return cloud_nn_ragged(a, a_offsets, b, b_offsets, batch, max_a, max_b, 0, out_dist, out_idx, scratch,
                           cloud_nn_scratch_bytes(batch, max_a, max_b, 0), (hipStream_t)stream);
}
int rald_post_cloud_metrics_ragged(const float* pred, const int64_t* pred_offsets, const float* gt, const int64_t* gt_offsets, int32_t batch,
                                   int64_t max_pred, int64_t max_gt, const double* thresholds_host, int32_t n_thresholds, double* out_raw,
                                   double* out_dist_pred, int64_t* out_idx_pred, double* out_dist_gt, int64_t* out_idx_gt, void* scratch,
                                   void* stream) {
    return cloud_metrics_ragged(pred, pred_offsets, gt, gt_offsets, batch, max_pred, max_gt, thresholds_host, n_thresholds, out_raw,
                                out_dist_pred, out_idx_pred, out_dist_gt, out_idx_gt, scratch, (hipStream_t)stream);
}
int64_t rald_op_nn_scratch_bytes(int32_t batch, int64_t max_a, int64_t max_b, int64_t b_chunk) {
    return cloud_nn_scratch_bytes(batch, max_a, max_b, b_chunk);
}
int rald_op_nn_ragged(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int32_t batch, int64_t max_a,
                      int64_t max_b, int64_t b_chunk, double* out_dist, int64_t* out_idx, void* scratch, int64_t scratch_bytes, void* stream) {
    return cloud_nn_ragged(a, a_offsets, b, b_offsets, batch, max_a, max_b, b_chunk, out_dist, out_idx, scratch, scratch_bytes, (hipStream_t)stream);
}

// ---- farthest-point sampling ------------------------------------------------------
int64_t rald_post_fps_scratch_bytes(int32_t batch, int64_t max_per_sample, int32_t form) {
    const int64_t n = fps_scratch_bytes(batch, max_per_sample, form);
    if (n < 0) set_error("rald_post_fps_scratch_bytes: batch >= 1, max_per_sample 1 .. 65536 (16384 for form 1), form 0 .. 2");
    return n;
}
int rald_post_fps_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                         int64_t max_per_sample, int32_t k, const int64_t* start, const float* scale3_host, int64_t* out_idx, float* out_dist2,
                         void* scratch, int64_t scratch_bytes, int32_t form, void* stream) {
    return fps_ragged(points, offsets, counts, batch, n_dense, max_per_sample, k, start, scale3_host, out_idx, out_dist2, scratch, scratch_bytes,
                      form, (hipStream_t)stream);
}

// ---- voxel-grid down-sampling ------------------------------------------------------
static const char* const kVoxelSizes =
    ": batch 1 .. 65535, n_total 0 .. 2^31 - 1, max_per_sample 1 .. 16777216, chunk 0 or a multiple of 1024";
int64_t rald_post_voxel_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample) {
    const int64_t n = voxel_scratch_bytes(batch, n_total, max_per_sample, 0);
    if (n < 0) set_error(std::string("rald_post_voxel_scratch_bytes") + kVoxelSizes);
    return n;
}
int rald_post_voxel_downsample_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                      int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                      const int32_t* dims3_host, float* out_points, int64_t* out_offsets, int32_t* out_count, int64_t* out_first,
                                      int32_t* out_cells, int64_t* out_inverse, void* scratch, int64_t scratch_bytes, void* stream) {
    return voxel_downsample_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                   out_points, out_offsets, out_count, out_first, out_cells, out_inverse, scratch, scratch_bytes, 0,
                                   (hipStream_t)stream);
}
int64_t rald_op_voxel_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t n = voxel_scratch_bytes(batch, n_total, max_per_sample, chunk);
    if (n < 0) set_error(std::string("rald_op_voxel_scratch_bytes") + kVoxelSizes);
    return n;
}
int32_t rald_op_voxel_passes(int64_t cells) {
    const int p = voxel_passes(cells);
    if (p < 0) set_error("rald_op_voxel_passes: cells must be 1 .. 2^31 - 1");
    return p;
}
int rald_op_voxel_downsample_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                    int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                    const int32_t* dims3_host, float* out_points, int64_t* out_offsets, int32_t* out_count, int64_t* out_first,
                                    int32_t* out_cells, int64_t* out_inverse, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream) {
    return voxel_downsample_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                   out_points, out_offsets, out_count, out_first, out_cells, out_inverse, scratch, scratch_bytes, chunk,
                                   (hipStream_t)stream);
}

// ---- fixed-radius neighbours and the radius outlier filter ------------------------------
int64_t rald_post_radius_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample) {
    const int64_t n = radius_scratch_bytes(batch, n_total, max_per_sample, 0);
    if (n < 0) set_error(std::string("rald_post_radius_scratch_bytes") + kVoxelSizes);
    return n;
}
int64_t rald_op_radius_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t n = radius_scratch_bytes(batch, n_total, max_per_sample, chunk);
    if (n < 0) set_error(std::string("rald_op_radius_scratch_bytes") + kVoxelSizes);
    return n;
}
int rald_post_radius_count_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                  const int32_t* dims3_host, float radius, int32_t max_count, int32_t* out_count, int64_t* out_nn_idx,
                                  float* out_nn_dist2, void* scratch, int64_t scratch_bytes, void* stream) {
    return radius_count_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                               radius, max_count, out_count, out_nn_idx, out_nn_dist2, scratch, scratch_bytes, 0, (hipStream_t)stream);
}
int rald_op_radius_count_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                const int32_t* dims3_host, float radius, int32_t max_count, int32_t* out_count, int64_t* out_nn_idx,
                                float* out_nn_dist2, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream) {
    return radius_count_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                               radius, max_count, out_count, out_nn_idx, out_nn_dist2, scratch, scratch_bytes, chunk, (hipStream_t)stream);
}
int rald_post_radius_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                   int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                   const int32_t* dims3_host, float radius, int32_t min_neighbors, float* out_points, int64_t* out_offsets,
                                   int64_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, void* stream) {
    return radius_filter_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                radius, min_neighbors, out_points, out_offsets, out_index, out_count, scratch, scratch_bytes, 0, (hipStream_t)stream);
}
int rald_op_radius_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                 int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                 const int32_t* dims3_host, float radius, int32_t min_neighbors, float* out_points, int64_t* out_offsets,
                                 int64_t* out_index, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream) {
    return radius_filter_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                radius, min_neighbors, out_points, out_offsets, out_index, out_count, scratch, scratch_bytes, chunk,
                                (hipStream_t)stream);
}

// ---- k nearest neighbours and the statistical outlier filter ------------------------------
int64_t rald_post_knn_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample) {
    const int64_t n = knn_scratch_bytes(batch, n_total, max_per_sample, 0);
    if (n < 0) set_error(std::string("rald_post_knn_scratch_bytes") + kVoxelSizes);
    return n;
}
int64_t rald_op_knn_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t n = knn_scratch_bytes(batch, n_total, max_per_sample, chunk);
    if (n < 0) set_error(std::string("rald_op_knn_scratch_bytes") + kVoxelSizes);
    return n;
}
int64_t rald_post_statistical_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample) {
    const int64_t n = statistical_scratch_bytes(batch, n_total, max_per_sample, 0);
    if (n < 0) set_error(std::string("rald_post_statistical_scratch_bytes") + kVoxelSizes);
    return n;
}
int64_t rald_op_statistical_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t n = statistical_scratch_bytes(batch, n_total, max_per_sample, chunk);
    if (n < 0) set_error(std::string("rald_op_statistical_scratch_bytes") + kVoxelSizes);
    return n;
}
int rald_post_knn_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense, int64_t n_total,
                         int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, int32_t k,
                         float max_radius, int64_t* out_idx, float* out_dist2, int32_t* out_found, void* scratch, int64_t scratch_bytes,
                         void* stream) {
    return knn_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                      k, max_radius, out_idx, out_dist2, out_found, scratch, scratch_bytes, 0, (hipStream_t)stream);
}
int rald_op_knn_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense, int64_t n_total,
                       int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, int32_t k,
                       float max_radius, int64_t* out_idx, float* out_dist2, int32_t* out_found, void* scratch, int64_t scratch_bytes,
                       int64_t chunk, void* stream) {
    return knn_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                      k, max_radius, out_idx, out_dist2, out_found, scratch, scratch_bytes, chunk, (hipStream_t)stream);
}
int rald_post_statistical_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                        int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                        const int32_t* dims3_host, int32_t k, float max_radius, double std_ratio, float* out_points,
                                        int64_t* out_offsets, int64_t* out_index, double* out_mean, double* out_stats, void* scratch,
                                        int64_t scratch_bytes, void* stream) {
    return statistical_filter_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                     k, max_radius, std_ratio, out_points, out_offsets, out_index, out_mean, out_stats, scratch, scratch_bytes, 0,
                                     (hipStream_t)stream);
}
int rald_op_statistical_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                      int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                      const int32_t* dims3_host, int32_t k, float max_radius, double std_ratio, float* out_points,
                                      int64_t* out_offsets, int64_t* out_index, double* out_mean, double* out_stats, void* scratch,
                                      int64_t scratch_bytes, int64_t chunk, void* stream) {
    return statistical_filter_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                     k, max_radius, std_ratio, out_points, out_offsets, out_index, out_mean, out_stats, scratch, scratch_bytes, chunk,
                                     (hipStream_t)stream);
}

// ---- PCA normals and normal consistency ------------------------------------------------
int64_t rald_post_normals_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample) {
    const int64_t n = normals_scratch_bytes(batch, n_total, max_per_sample, 0);
    if (n < 0) set_error(std::string("rald_post_normals_scratch_bytes") + kVoxelSizes);
    return n;
}
int64_t rald_op_normals_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t n = normals_scratch_bytes(batch, n_total, max_per_sample, chunk);
    if (n < 0) set_error(std::string("rald_op_normals_scratch_bytes") + kVoxelSizes);
    return n;
}
int rald_post_normals_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                             int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host,
                             int32_t k, float max_radius, const float* view3_host, float* out_normals, float* out_curvature,
                             float* out_eigenvalues, int32_t* out_found, void* scratch, int64_t scratch_bytes, void* stream) {
    return normals_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host}, k,
                          max_radius, view3_host, out_normals, out_curvature, out_eigenvalues, out_found, scratch, scratch_bytes, 0,
                          (hipStream_t)stream);
}
int rald_op_normals_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense, int64_t n_total,
                           int64_t max_per_sample, const float* lo3_host, const float* v3_host, const int32_t* dims3_host, int32_t k,
                           float max_radius, const float* view3_host, float* out_normals, float* out_curvature, float* out_eigenvalues,
                           int32_t* out_found, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream) {
    return normals_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host}, k,
                          max_radius, view3_host, out_normals, out_curvature, out_eigenvalues, out_found, scratch, scratch_bytes, chunk,
                          (hipStream_t)stream);
}
int64_t rald_post_normal_consistency_scratch_bytes(int32_t batch, int64_t n_pred_total, int64_t n_gt_total, int64_t max_pred, int64_t max_gt) {
    const int64_t n = normal_consistency_scratch_bytes(batch, n_pred_total, n_gt_total, max_pred, max_gt);
    if (n < 0) set_error("rald_post_normal_consistency_scratch_bytes: batch 1 .. 65535, the totals and the bounds 0 .. 2^31 - 1");
    return n;
}
int rald_post_normal_consistency_ragged(const float* pred, const float* pred_normals, const int64_t* pred_offsets, int64_t n_pred_total,
                                        const float* gt, const float* gt_normals, const int64_t* gt_offsets, int64_t n_gt_total, int32_t batch,
                                        int64_t max_pred, int64_t max_gt, double* out_nc, int64_t* out_counts, void* scratch,
                                        int64_t scratch_bytes, void* stream) {
    return normal_consistency_ragged(pred, pred_normals, pred_offsets, n_pred_total, gt, gt_normals, gt_offsets, n_gt_total, batch, max_pred,
                                     max_gt, out_nc, out_counts, scratch, scratch_bytes, (hipStream_t)stream);
}

// ---- density clustering and small-cluster removal ----------------------------------------
int64_t rald_post_cluster_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample) {
    const int64_t n = cluster_scratch_bytes(batch, n_total, max_per_sample, 0);
    if (n < 0) set_error(std::string("rald_post_cluster_scratch_bytes") + kVoxelSizes);
    return n;
}
int64_t rald_op_cluster_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    const int64_t n = cluster_scratch_bytes(batch, n_total, max_per_sample, chunk);
    if (n < 0) set_error(std::string("rald_op_cluster_scratch_bytes") + kVoxelSizes);
    return n;
}
int rald_post_cluster_labels_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                    int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                    const int32_t* dims3_host, float eps, int32_t min_points, int32_t* out_labels, int32_t* out_num_clusters,
                                    int32_t* out_sizes, int32_t* out_count, void* scratch, int64_t scratch_bytes, void* stream) {
    return cluster_labels_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                 eps, min_points, out_labels, out_num_clusters, out_sizes, out_count, scratch, scratch_bytes, 0,
                                 (hipStream_t)stream);
}
int rald_op_cluster_labels_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                  const int32_t* dims3_host, float eps, int32_t min_points, int32_t* out_labels, int32_t* out_num_clusters,
                                  int32_t* out_sizes, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream) {
    return cluster_labels_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                 eps, min_points, out_labels, out_num_clusters, out_sizes, out_count, scratch, scratch_bytes, chunk,
                                 (hipStream_t)stream);
}
int rald_post_cluster_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                    int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                    const int32_t* dims3_host, float eps, int32_t min_points, int32_t min_cluster_size, int32_t largest_only,
                                    float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, int32_t* out_num_clusters,
                                    void* scratch, int64_t scratch_bytes, void* stream) {
    return cluster_filter_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                 eps, min_points, min_cluster_size, largest_only, out_points, out_offsets, out_index, out_labels,
                                 out_num_clusters, scratch, scratch_bytes, 0, (hipStream_t)stream);
}
int rald_op_cluster_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, const float* lo3_host, const float* v3_host,
                                  const int32_t* dims3_host, float eps, int32_t min_points, int32_t min_cluster_size, int32_t largest_only,
                                  float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, int32_t* out_num_clusters,
                                  void* scratch, int64_t scratch_bytes, int64_t chunk, void* stream) {
    return cluster_filter_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), {lo3_host, v3_host, dims3_host},
                                 eps, min_points, min_cluster_size, largest_only, out_points, out_offsets, out_index, out_labels,
                                 out_num_clusters, scratch, scratch_bytes, chunk, (hipStream_t)stream);
}

// ---- RANSAC plane segmentation and plane removal ------------------------------------------
int64_t rald_post_plane_scratch_bytes(int32_t batch, int64_t n_total, int64_t max_per_sample, int32_t num_hypotheses, int32_t max_planes) {
    const int64_t n = plane_scratch_bytes(batch, n_total, max_per_sample, num_hypotheses, max_planes);
    if (n < 0)
        set_error("rald_post_plane_scratch_bytes: batch 1 .. 65535, n_total 0 .. 2^31 - 1, max_per_sample 1 .. 2^24, num_hypotheses 1 .. 65536, "
                  "max_planes 1 .. 8");
    return n;
}
int rald_post_plane_segment_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                   int64_t n_total, int64_t max_per_sample, float threshold, int32_t num_hypotheses, int32_t max_planes,
                                   int32_t min_inliers, int32_t refine, int64_t seed, const float* view3_host, int32_t* out_labels,
                                   double* out_planes, int32_t* out_num_planes, int32_t* out_inliers, int32_t* out_best, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
    return plane_segment_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), threshold, num_hypotheses,
                                max_planes, min_inliers, refine, seed, view3_host, out_labels, out_planes, out_num_planes, out_inliers, out_best,
                                scratch, scratch_bytes, (hipStream_t)stream);
}
int rald_post_plane_filter_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                  int64_t n_total, int64_t max_per_sample, float threshold, int32_t num_hypotheses, int32_t max_planes,
                                  int32_t min_inliers, int32_t refine, int64_t seed, const float* view3_host, int32_t keep_planes,
                                  float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, double* out_planes,
                                  int32_t* out_num_planes, void* scratch, int64_t scratch_bytes, void* stream) {
    return plane_filter_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), threshold, num_hypotheses,
                               max_planes, min_inliers, refine, seed, view3_host, keep_planes, out_points, out_offsets, out_index, out_labels,
                               out_planes, out_num_planes, scratch, scratch_bytes, (hipStream_t)stream);
}

// ---- ICP registration and rigid transforms -------------------------------------------------
int64_t rald_op_icp_scratch_bytes(int32_t batch, int64_t n_src_total, int64_t max_src, int64_t n_tgt_total, int64_t max_tgt, int64_t chunk) {
    const int64_t n = icp_scratch_bytes(batch, n_src_total, max_src, n_tgt_total, max_tgt, chunk);
    if (n < 0)
        set_error("rald_post_icp_scratch_bytes: batch 1 .. 65535, n_src_total and n_tgt_total 0 .. 2^31 - 1, max_src and max_tgt 1 .. 2^24, "
                  "chunk 0 or a multiple of 1024");
    return n;
}
int64_t rald_post_icp_scratch_bytes(int32_t batch, int64_t n_src_total, int64_t max_src, int64_t n_tgt_total, int64_t max_tgt) {
    return rald_op_icp_scratch_bytes(batch, n_src_total, max_src, n_tgt_total, max_tgt, 0);
}
int rald_op_icp_ragged(const float* source, const int64_t* src_offsets, const int32_t* src_counts, int64_t src_n_dense, int64_t n_src_total,
                       int64_t max_src, const float* target, const int64_t* tgt_offsets, const int32_t* tgt_counts, int64_t tgt_n_dense,
                       int64_t n_tgt_total, int64_t max_tgt, const float* target_normals, int32_t batch, const float* lo3_host,
                       const float* v3_host, const int32_t* dims3_host, int32_t mode, float max_distance, int32_t max_iterations,
                       double tolerance, int32_t min_correspondences, const double* init, double* out_transform, double* out_stats,
                       int32_t* out_info, int64_t* out_corr, float* out_moved, void* scratch, int64_t scratch_bytes, int64_t chunk,
                       void* stream) {
    return icp_ragged(ragged_cloud(source, src_offsets, src_counts, batch, src_n_dense, n_src_total, max_src),
                      ragged_cloud(target, tgt_offsets, tgt_counts, batch, tgt_n_dense, n_tgt_total, max_tgt), target_normals,
                      {lo3_host, v3_host, dims3_host}, mode, max_distance, max_iterations, tolerance, min_correspondences, init, out_transform,
                      out_stats, out_info, out_corr, out_moved, scratch, scratch_bytes, chunk, (hipStream_t)stream);
}
int rald_post_icp_ragged(const float* source, const int64_t* src_offsets, const int32_t* src_counts, int64_t src_n_dense, int64_t n_src_total,
                         int64_t max_src, const float* target, const int64_t* tgt_offsets, const int32_t* tgt_counts, int64_t tgt_n_dense,
                         int64_t n_tgt_total, int64_t max_tgt, const float* target_normals, int32_t batch, const float* lo3_host,
                         const float* v3_host, const int32_t* dims3_host, int32_t mode, float max_distance, int32_t max_iterations,
                         double tolerance, int32_t min_correspondences, const double* init, double* out_transform, double* out_stats,
                         int32_t* out_info, int64_t* out_corr, float* out_moved, void* scratch, int64_t scratch_bytes, void* stream) {
    return rald_op_icp_ragged(source, src_offsets, src_counts, src_n_dense, n_src_total, max_src, target, tgt_offsets, tgt_counts, tgt_n_dense,
                              n_tgt_total, max_tgt, target_normals, batch, lo3_host, v3_host, dims3_host, mode, max_distance, max_iterations,
                              tolerance, min_correspondences, init, out_transform, out_stats, out_info, out_corr, out_moved, scratch,
                              scratch_bytes, 0, stream);
}
int rald_post_rigid_transform_ragged(const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int64_t n_dense,
                                     int64_t n_total, int64_t max_per_sample, const double* transforms, int32_t transform_stride,
                                     const float* normals, float* out_points, float* out_normals, void* stream) {
    return rigid_transform_ragged(ragged_cloud(points, offsets, counts, batch, n_dense, n_total, max_per_sample), transforms, transform_stride,
                                  normals, out_points, out_normals, (hipStream_t)stream);
}

// ---- isosurface meshing of dense volumes by surface nets ---------------------------------
int64_t rald_post_surface_scratch_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t nz) {
    const int64_t n = surface_scratch_bytes(batch, nx, ny, nz);
    if (n < 0) set_error("rald_post_surface_scratch_bytes: batch 1 .. 65535, dims 2 .. 1024 each, batch * nx * ny * nz <= 357913941");
    return n;
}
int rald_post_surface_nets(const float* volume, int32_t batch, const int32_t* dims3_host, const float* lo3_host, const float* spacing3_host,
                           float iso, float* out_vertices, int64_t* out_v_offsets, int64_t max_vertices, int32_t* out_faces,
                           int64_t* out_f_offsets, int64_t max_faces, int32_t* out_cells, void* scratch, int64_t scratch_bytes, void* stream) {
    return surface_nets(volume, batch, dims3_host, lo3_host, spacing3_host, iso, out_vertices, out_v_offsets, max_vertices, out_faces,
                        out_f_offsets, max_faces, out_cells, scratch, scratch_bytes, (hipStream_t)stream);
}

int rald_radar_cube_prepare(const float* raw, int32_t batch, int32_t R, int32_t A, int32_t E, int32_t raw_channels, int32_t tgt_A,
                            int32_t tgt_E, int32_t norm_intensity, float max_intensity, int32_t norm_dopp, float max_dopp, float* out,
                            void* stream) {
    return radar_cube_prepare(raw, batch, R, A, E, raw_channels, tgt_A, tgt_E, norm_intensity, max_intensity, norm_dopp, max_dopp, out,
                              (hipStream_t)stream);
}

// ---- radar front end: ADC frames -> RAEIVV cubes (radar_dsp.hip) ---------------------------------
struct rald_radar_dsp { RadarDsp* impl; };
int rald_radar_dsp_create(const rald_radar_dsp_config* cfg, const int32_t* tx_layout, const int32_t* rx_layout, const double* vbins,
                          int32_t n_vbins, rald_radar_dsp** out) {
    RALD_CHECK(cfg && out, "rald_radar_dsp_create: null argument");
    RadarDsp* impl = nullptr;
    RALD_TRY(radar_dsp_create(*cfg, tx_layout, rx_layout, vbins, n_vbins, &impl));
    *out = new rald_radar_dsp{impl};
    return 0;
}
void rald_radar_dsp_destroy(rald_radar_dsp* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h->impl;
    delete h;
}
int64_t rald_radar_dsp_workspace_bytes(const rald_radar_dsp_config* cfg, int32_t batch) {
    if (!cfg || batch < 1 || radar_dsp_check_sizes(*cfg)) return -1;
    return radar_dsp_workspace_bytes(*cfg, batch);
}
int rald_radar_dsp_run(const rald_radar_dsp* h, const void* frames, int32_t input_kind, int32_t batch, float* out, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    RALD_CHECK(h, "rald_radar_dsp_run: null handle");
    return radar_dsp_run(*h->impl, frames, input_kind, batch, out, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- helper points: intensity cubes -> CFAR query points (radar_points.hip) -----------------------
struct rald_radar_points { RadarPoints* impl; };
int rald_radar_points_create(const rald_radar_points_config* cfg, const float* axis_r, const float* axis_a, const float* axis_e,
                             const uint8_t* keep_r, const uint8_t* keep_a, const uint8_t* keep_e, rald_radar_points** out) {
    RALD_CHECK(cfg && out, "rald_radar_points_create: null argument");
    RadarPoints* impl = nullptr;
    RALD_TRY(radar_points_create(*cfg, axis_r, axis_a, axis_e, keep_r, keep_a, keep_e, &impl));
    *out = new rald_radar_points{impl};
    return 0;
}
void rald_radar_points_destroy(rald_radar_points* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h->impl;
    delete h;
}
int64_t rald_radar_points_workspace_bytes(const rald_radar_points_config* cfg, int32_t batch) {
    if (!cfg || batch < 1 || radar_points_check_config(*cfg)) return -1;
    return radar_points_workspace_bytes(*cfg, batch);
}
int rald_radar_points_run(const rald_radar_points* h, const float* cubes, int32_t batch, float* points, int32_t* counts, int32_t* peaks,
                          float* intensities, void* workspace, int64_t workspace_bytes, void* stream) {
    RALD_CHECK(h, "rald_radar_points_run: null handle");
    return radar_points_run(*h->impl, cubes, batch, points, counts, peaks, intensities, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- LiDAR front end: scans -> voxels -> occupancy queries (lidar.hip) ----------------------------
struct rald_lidar { Lidar impl; };
int rald_lidar_create(const rald_lidar_config* cfg, rald_lidar** out) {
    RALD_CHECK(cfg && out, "rald_lidar_create: null argument");
    Lidar impl;
    RALD_TRY(lidar_check_config(*cfg, &impl));
    *out = new rald_lidar{impl};
    return 0;
}
void rald_lidar_destroy(rald_lidar* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h;
}
int64_t rald_lidar_workspace_bytes(const rald_lidar_config* cfg, int32_t batch, int64_t total_points) {
    Lidar impl;
    if (!cfg || batch < 1 || total_points < 0 || lidar_check_config(*cfg, &impl)) return -1;
    return lidar_workspace_bytes(impl, batch, total_points);
}
int rald_lidar_crop(const rald_lidar* h, const float* points, int32_t in_stride, const int64_t* offsets, int32_t batch, float* out,
                    int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
    RALD_CHECK(h, "rald_lidar_crop: null handle");
    return lidar_crop(h->impl, points, in_stride, offsets, batch, out, counts, workspace, workspace_bytes, (hipStream_t)stream);
}
int rald_lidar_voxelize(const rald_lidar* h, const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch,
                        int32_t to_polar, float* polar_out, float* voxels, int32_t* coords, int32_t* num_points, int32_t* kept_keys,
                        int32_t* voxel_counts, void* workspace, int64_t workspace_bytes, void* stream) {
    RALD_CHECK(h, "rald_lidar_voxelize: null handle");
    return lidar_voxelize(h->impl, points, offsets, counts, batch, to_polar, polar_out, voxels, coords, num_points, kept_keys, voxel_counts,
                          workspace, workspace_bytes, (hipStream_t)stream);
}
int rald_lidar_queries(const rald_lidar* h, const float* points, const int64_t* offsets, int32_t batch, int32_t num_samples,
                       int32_t in_num, const int64_t* sample_idx, const double* u_in, const int64_t* voxel_idx, const double* u_out,
                       const int64_t* empty_rank, const int32_t* coords, const int32_t* kept_keys, const int32_t* voxel_counts,
                       float* lidar_points, float* query_points, float* query_labels, void* workspace, int64_t workspace_bytes,
                       void* stream) {
    RALD_CHECK(h, "rald_lidar_queries: null handle");
    return lidar_queries(h->impl, points, offsets, batch, num_samples, in_num, sample_idx, u_in, voxel_idx, u_out, empty_rank, coords,
                         kept_keys, voxel_counts, lidar_points, query_points, query_labels, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- query generation + refine --------------------------------------------------
int rald_query_uniform(const double* u3n, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy,
                       float* out_queries, void* stream) {
    RALD_CHECK(pc_range6_host && (n == 0 || (u3n && out_queries)), "rald_query_uniform: null argument");
    return query_uniform(u3n, n, pc_range6_host, norm_anisotropy, norm_isotropy, out_queries, (hipStream_t)stream);
}
int rald_query_uniform_cart(const double* u3n, int64_t n, const double* pc_range_cart6_host, const double* pc_range6_host,
                            int32_t norm_anisotropy, int32_t norm_isotropy, float* out_queries, int64_t* out_count, void* scratch,
                            void* stream) {
    RALD_CHECK(pc_range_cart6_host && pc_range6_host && out_count && (n == 0 || (u3n && out_queries && scratch)),
               "rald_query_uniform_cart: null argument");
    return query_uniform_cart(u3n, n, pc_range_cart6_host, pc_range6_host, norm_anisotropy, norm_isotropy, out_queries, out_count,
                              (int*)scratch, (hipStream_t)stream);
}
int rald_query_norm_points(const float* points, int64_t n, const double* pc_range6_host, int32_t norm_anisotropy, int32_t norm_isotropy,
                           float* out_points, void* stream) {
    RALD_CHECK(pc_range6_host && (n == 0 || (points && out_points)), "rald_query_norm_points: null argument");
    return query_norm_points(points, n, pc_range6_host, norm_anisotropy, norm_isotropy, out_points, (hipStream_t)stream);
}
int rald_query_grid(const float* lo3_host, const float* spacing3_host, const int32_t* dims3_host, int32_t i0, int32_t ni, float* out_points,
                    void* stream) {
    return query_grid(lo3_host, spacing3_host, dims3_host, i0, ni, out_points, (hipStream_t)stream);
}
int rald_query_refine(const float* helper_points, int64_t n_helper, int64_t aug_num, const int64_t* sel_index, const int64_t* aug_scales,
                      const double* u_bias, const double* pc_range6_host, const double* voxel_size3_host, int32_t norm_anisotropy,
                      int32_t norm_isotropy, int32_t normalise, float* out_points, void* stream) {
    RALD_CHECK(pc_range6_host && voxel_size3_host && (aug_num == 0 || (helper_points && out_points)), "rald_query_refine: null argument");
    return query_refine(helper_points, n_helper, aug_num, sel_index, aug_scales, u_bias, pc_range6_host, voxel_size3_host, norm_anisotropy,
                        norm_isotropy, normalise, out_points, (hipStream_t)stream);
}
int rald_query_refine_ragged(const float* points, const int64_t* offsets, int32_t batch, int64_t aug_num, const int64_t* sel_index,
                             const double* u_sel, const int64_t* aug_scales, const double* u_bias, const double* pc_range6_host,
                             const double* voxel_size3_host, int32_t norm_anisotropy, int32_t norm_isotropy, int32_t normalise,
                             float* out_queries, int64_t* out_offsets, void* stream) {
    return query_refine_ragged(points, offsets, batch, aug_num, sel_index, u_sel, aug_scales, u_bias, pc_range6_host, voxel_size3_host,
                               norm_anisotropy, norm_isotropy, normalise, out_queries, out_offsets, (hipStream_t)stream);
}

// ---- optimizer step on flat parameter storage --------------------------------------
int rald_optim_grad_sumsq(const float* grads, int64_t n, double* out_sumsq, void* stream) {
    RALD_CHECK(out_sumsq && (n == 0 || grads), "rald_optim_grad_sumsq: null argument");
    return optim_grad_sumsq(grads, n, out_sumsq, (hipStream_t)stream);
}
int rald_optim_clip_coef(const double* sumsq, float pre_scale, float max_norm, float* out_norm_coef, void* stream) {
    RALD_CHECK(sumsq && out_norm_coef, "rald_optim_clip_coef: null argument");
    return optim_clip_coef(sumsq, pre_scale, max_norm, out_norm_coef, (hipStream_t)stream);
}
int rald_optim_adamw_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema_params, int64_t n,
                         const float* grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                         double ema_rate, int32_t write_back_grads, void* stream) {
    RALD_CHECK(n == 0 || (params && grads && exp_avg && exp_avg_sq), "rald_optim_adamw_ema: null argument");
    return optim_adamw_ema(params, grads, exp_avg, exp_avg_sq, ema_params, n, grad_scale, lr, beta1, beta2, eps, weight_decay, step, ema_rate,
                           write_back_grads, (hipStream_t)stream);
}
int rald_optim_ema(float* ema_params, const float* params, int64_t n, double rate, void* stream) {
    RALD_CHECK(n == 0 || (ema_params && params), "rald_optim_ema: null argument");
    return optim_ema(ema_params, params, n, rate, (hipStream_t)stream);
}

// ---- kernel-level entry points -----------------------------------------------------------------
int rald_op_gemm_nt(const void* A, int64_t lda, int64_t strideA, const void* B, int64_t ldb, int64_t strideB,
                    void* C, int64_t ldc, int64_t strideC, const float* bias, int32_t M, int32_t N, int32_t K,
                    int32_t batch, float alpha, int32_t epilogue, void* stream) {
    RALD_CHECK(A && B && C, "rald_op_gemm_nt: null pointer");
    GemmArgs g;
    g.A = (const bf16*)A; g.lda = lda; g.strideA = strideA; g.B = (const bf16*)B; g.ldb = ldb; g.strideB = strideB;
    g.C = C; g.ldc = ldc; g.strideC = strideC; g.bias = bias; g.M = M; g.N = N; g.K = K; g.batch = batch; g.alpha = alpha; g.alpha_ncols = 1 << 30; g.flags = 0;
    return gemm_nt(g, epilogue, (hipStream_t)stream);
}
int rald_op_gemm_nt2(const void* A, int64_t lda, int64_t strideA, int64_t strideA2, const void* B, int64_t ldb, int64_t strideB, int64_t strideB2,
                     void* C, int64_t ldc, int64_t strideC, int64_t strideC2, const float* bias, int32_t M, int32_t N, int32_t K, int32_t batch,
                     int32_t batch2, float alpha, int32_t epilogue, void* stream) {
    RALD_CHECK(A && B && C, "rald_op_gemm_nt2: null pointer");
    GemmArgs g = gemm_args((const bf16*)A, lda, (const bf16*)B, ldb, C, ldc, bias, M, N, K);
    g.strideA = strideA; g.strideB = strideB; g.strideC = strideC; g.batch = batch; g.alpha = alpha;
    g.batch2 = batch2; g.strideA2 = strideA2; g.strideB2 = strideB2; g.strideC2 = strideC2;
    return gemm_nt(g, epilogue, (hipStream_t)stream);
}
int rald_op_gemm_nt_256(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const float* bias, int32_t M, int32_t N,
                        int32_t K, float alpha, int32_t alpha_ncols, int32_t epilogue, int32_t persistent, int32_t max_workgroups, void* stream) {
    RALD_CHECK(A && B && C, "rald_op_gemm_nt_256: null pointer");
    GemmArgs g = gemm_args((const bf16*)A, lda, (const bf16*)B, ldb, C, ldc, bias, M, N, K);
    g.alpha = alpha; g.alpha_ncols = alpha_ncols;
    return gemm_nt_256_test(g, epilogue, persistent, max_workgroups, (hipStream_t)stream);
}
int rald_op_gemm_nt_256_batched(const void* A, int64_t lda, int64_t strideA, const void* B, int64_t ldb, int64_t strideB, void* C, int64_t ldc,
                                int64_t strideC, const float* bias, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t batch2, float alpha,
                                int32_t alpha_ncols, int32_t epilogue, int32_t persistent, int32_t max_workgroups, void* stream) {
    RALD_CHECK(A && B && C, "rald_op_gemm_nt_256_batched: null pointer");
    GemmArgs g = gemm_args((const bf16*)A, lda, (const bf16*)B, ldb, C, ldc, bias, M, N, K);
    g.strideA = strideA; g.strideB = strideB; g.strideC = strideC; g.batch = batch; g.batch2 = batch2;
    g.alpha = alpha; g.alpha_ncols = alpha_ncols;
    return gemm_nt_256_batched_test(g, epilogue, persistent, max_workgroups, (hipStream_t)stream);
}
int rald_op_gemm_tn(const void* A_bf16, int64_t lda, const void* B_bf16, int64_t ldb, float* C, int64_t ldc, float* colsum, int32_t M, int32_t N1,
                    int32_t N2, void* workspace, int64_t workspace_bytes, void* stream) {
    return gemm_tn((const bf16*)A_bf16, lda, (const bf16*)B_bf16, ldb, C, ldc, colsum, M, N1, N2, (hipStream_t)stream, (float*)workspace, workspace_bytes / 4);
}
int rald_op_conv3d_wgrad(const void* dy_bf16, const void* x_bf16, float* dW, float* dbias, int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin,
                         int32_t Cout, int32_t stride, int32_t pad, void* workspace, int64_t workspace_bytes, void* stream) {
    return conv3d_wgrad_tn((const bf16*)dy_bf16, (const bf16*)x_bf16, dW, dbias, B, ID, IH, IW, Cin, Cout, stride, pad, (hipStream_t)stream, (float*)workspace,
                           workspace_bytes / 4);
}
int64_t rald_op_gemm_tn_workspace_bytes(int32_t M, int32_t N1, int32_t N2) { return 4 * gemm_tn_workspace_floats(M, N1, N2); }
int64_t rald_op_conv3d_wgrad_workspace_bytes(int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad) {
    return 4 * conv3d_wgrad_workspace_floats(B, ID, IH, IW, Cin, Cout, stride, pad);
}
int rald_op_conv3d_wgrad_route(int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad, int32_t* ranges_out,
                               int32_t* per_range_out) {
    int ranges = 0, per_range = 0;
    const int r = conv3d_wgrad_route(B, ID, IH, IW, Cin, Cout, stride, pad, &ranges, &per_range);
    if (r < 0) set_error("rald_op_conv3d_wgrad_route: not a shape rald_op_conv3d_wgrad takes (Cin % 8, Cout % 8, stride 1|2, pad >= 0, < 2^31 output voxels)");
    if (ranges_out) *ranges_out = ranges;
    if (per_range_out) *per_range_out = per_range;
    return r;
}
int rald_op_patches27(const float* cube, int32_t cube_ch, void* out_bf16, int32_t B, int32_t D, int32_t H, int32_t W, void* stream) {
    return patches27(cube, cube_ch, (bf16*)out_bf16, B, D, H, W, (hipStream_t)stream);
}
int rald_op_transpose(const void* in, int32_t in_is_bf16, int64_t ld_in, int64_t stride_in, int64_t stride_in2, void* out_bf16, int64_t ld_out,
                      int64_t stride_out, int64_t stride_out2, int32_t rows, int32_t cols, int32_t batch, int32_t batch2, void* stream) {
    TransposeArgs a;
    a.in = in; a.ld_in = ld_in; a.stride_in = stride_in; a.stride_in2 = stride_in2; a.out = (bf16*)out_bf16; a.ld_out = ld_out;
    a.stride_out = stride_out; a.stride_out2 = stride_out2; a.rows = rows; a.cols = cols; a.batch = batch; a.batch2 = batch2;
    return transpose_rows(a, in_is_bf16, (hipStream_t)stream);
}
int rald_op_ln_mod_bwd(const float* x, const float* dh, const float* scale, int64_t gstride, int32_t rows_per_group, float add_one, float eps,
                       int64_t rows, int32_t D, float* dx_accum, void* dx_bf16_out, float* dscale_accum, float* dshift_accum, void* stream) {
    RALD_CHECK(x && dh && scale && dx_accum && dscale_accum && dshift_accum, "rald_op_ln_mod_bwd: null pointer");
    return ln_mod_bwd(x, dh, scale, gstride, rows_per_group, add_one, eps, rows, D, dx_accum, dscale_accum, dshift_accum, (hipStream_t)stream, (bf16*)dx_bf16_out);
}
int rald_op_geglu_fwd(const void* u_bf16, void* hid_bf16, int64_t M, int32_t inner, void* stream) {
    RALD_CHECK(u_bf16 && hid_bf16, "rald_op_geglu_fwd: null pointer");
    return geglu_fwd((const bf16*)u_bf16, (bf16*)hid_bf16, M, inner, (hipStream_t)stream);
}
int rald_op_geglu_bwd(const void* u_bf16, const void* dhid_bf16, void* du_bf16, int64_t M, int32_t inner, void* stream) {
    RALD_CHECK(u_bf16 && dhid_bf16 && du_bf16, "rald_op_geglu_bwd: null pointer");
    return geglu_bwd((const bf16*)u_bf16, (const bf16*)dhid_bf16, (bf16*)du_bf16, M, inner, (hipStream_t)stream);
}
int rald_op_colsum(const void* X, int32_t is_bf16, int64_t ld, int64_t M, int32_t N, float* out_accum, void* stream) {
    return colsum(X, is_bf16, ld, M, N, out_accum, (hipStream_t)stream);
}
int rald_op_row_lse(const float* S, int64_t rows, int32_t cols, float scale, float* lse, void* stream) {
    RALD_CHECK(S && lse, "rald_op_row_lse: null pointer");
    return row_lse(S, rows, cols, scale, lse, (hipStream_t)stream);
}
int rald_op_rowdot_heads(const void* dO_bf16, const void* O_bf16, int64_t M, int32_t heads, int32_t nq, float* delta, void* stream) {
    RALD_CHECK(dO_bf16 && O_bf16 && delta, "rald_op_rowdot_heads: null pointer");
    return rowdot_heads((const bf16*)dO_bf16, (const bf16*)O_bf16, M, heads, nq, delta, (hipStream_t)stream);
}
int rald_op_attn_bwd_elem(const float* S, const float* dP, const float* lse, const float* delta, int64_t batch, int32_t R, int32_t Ccols,
                          int64_t vbatch_stride, int32_t vstride, float scale, int32_t by_col, void* P_bf16, void* dS_bf16, void* stream) {
    RALD_CHECK(S && dP && lse && delta && dS_bf16, "rald_op_attn_bwd_elem: null pointer");
    return attn_bwd_elem(S, dP, lse, delta, batch, R, Ccols, vbatch_stride, vstride, scale, by_col, (bf16*)P_bf16, (bf16*)dS_bf16, (hipStream_t)stream);
}
int rald_op_sgemm_acc(const float* A, int64_t lda, int32_t trans_a, const float* B, int64_t ldb, int32_t trans_b, float* C, int64_t ldc, int32_t M,
                      int32_t N, int32_t K, float alpha, void* stream) {
    return sgemm_acc(A, lda, trans_a, B, ldb, trans_b, C, ldc, M, N, K, alpha, (hipStream_t)stream);
}
int rald_op_silu_fwd(const float* x, float* y, int64_t n, void* stream) { return silu_fwd(x, y, n, (hipStream_t)stream); }
int rald_op_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) { return silu_bwd(x, dy, dx, n, (hipStream_t)stream); }
int rald_op_posemb(const float* t, float* out, int32_t n, int32_t channels, void* stream) {
    RALD_CHECK(t && out && n > 0, "rald_op_posemb: bad arguments");
    return positional_embedding(t, out, n, channels, (hipStream_t)stream);
}
int rald_op_edm_loss_grad(const float* F, const float* x_noised, const float* y, const float* coef3, int64_t per_sample, int64_t total, float* dF,
                          float* D_out, double* loss, void* stream) {
    RALD_CHECK(F && x_noised && y && coef3 && dF && loss, "rald_op_edm_loss_grad: null pointer");
    return edm_loss_grad(F, x_noised, y, coef3, per_sample, total, dF, D_out, loss, (hipStream_t)stream);
}
// ---- radar encoder, op level (forward pieces + backward building blocks) --------------------------------------
int rald_op_conv3d(const void* in_bf16, const void* w_packed_bf16, const float* bias, const float* resid, float* out, void* out_bf16, int32_t B,
                   int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad, void* stream) {
    return conv3d_igemm((const bf16*)in_bf16, (const bf16*)w_packed_bf16, bias, resid, out, B, ID, IH, IW, Cin, Cout, stride, pad, (hipStream_t)stream,
                        (bf16*)out_bf16);
}
int rald_op_conv3d_route(int32_t B, int32_t ID, int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad, int32_t allow_split,
                         int32_t* splits_out) {
    if (splits_out) *splits_out = 0;
    if (!(B > 0 && ID > 0 && IH > 0 && IW > 0 && (stride == 1 || stride == 2) && ID >= stride && IH >= stride && IW >= stride && Cin > 0 &&
          Cin % 64 == 0 && Cout > 0 && Cout % 4 == 0 && pad >= 0 && pad <= 2 && (allow_split == 0 || allow_split == 1))) {
        set_error("rald_op_conv3d_route: not a shape rald_op_conv3d_full takes (Cin % 64, Cout % 4, stride 1|2, pad 0..2, allow_split 0|1)");
        return -1;
    }
    const ConvRoute r = conv3d_route(B, ID, IH, IW, Cin, Cout, stride, pad, allow_split);
    if (splits_out) *splits_out = r.splits;
    return r.engine;
}
int rald_op_conv3d_full(const void* in_bf16, const void* w_packed_bf16, const float* bias, const float* resid, float* out, void* out_bf16,
                        double* gn_part, void* split_workspace, int64_t split_workspace_bytes, int32_t allow_split, int32_t B, int32_t ID,
                        int32_t IH, int32_t IW, int32_t Cin, int32_t Cout, int32_t stride, int32_t pad, void* stream) {
    return conv3d_full((const bf16*)in_bf16, (const bf16*)w_packed_bf16, bias, resid, out, (bf16*)out_bf16, gn_part, (float*)split_workspace,
                       split_workspace_bytes, allow_split, B, ID, IH, IW, Cin, Cout, stride, pad, (hipStream_t)stream);
}
int rald_op_gn_finish(const double* part, double* stats, int32_t B, int32_t nblk, void* stream) {
    return gn_finish(part, stats, B, nblk, (hipStream_t)stream);
}
int rald_op_upsample2_cast(const float* x, void* y_bf16, int32_t B, int32_t D, int32_t H, int32_t W, int32_t C, void* stream) {
    return upsample2_cast(x, (bf16*)y_bf16, B, D, H, W, C, (hipStream_t)stream);
}
int rald_op_pad_cast64(const float* z, void* y_bf16, int64_t rows, int32_t zc, void* stream) {
    return pad_cast64(z, (bf16*)y_bf16, rows, zc, (hipStream_t)stream);
}
int rald_op_radar_tokens(const float* z, const float* Wp, const float* bp, const float* r_emb, const float* a_emb, const float* e_emb, float* tokens,
                         int32_t B, int32_t R, int32_t A, int32_t E, int32_t zc, int32_t C, void* stream) {
    return radar_tokens(z, Wp, bp, r_emb, a_emb, e_emb, tokens, B, R, A, E, zc, C, (hipStream_t)stream);
}
int rald_op_groupnorm(const float* x, const float* gamma, const float* beta, void* y_bf16, double* stats, int32_t B, int32_t S, int32_t C,
                      int32_t swish, void* stream) {
    return groupnorm_fwd(x, gamma, beta, (bf16*)y_bf16, stats, B, S, C, swish, (hipStream_t)stream);
}
int rald_op_groupnorm_bwd(const float* x, const double* stats, const float* gamma, const float* beta, const void* da, int32_t da_is_bf16, float* dx,
                          void* dx_bf16, float* dgamma, float* dbeta, double* gsum_scratch, int32_t B, int32_t S, int32_t C, int32_t swish,
                          int32_t accumulate, void* stream) {
    return groupnorm_bwd(x, stats, gamma, beta, (const float*)da, dx, dgamma, dbeta, gsum_scratch, B, S, C, swish, accumulate, (hipStream_t)stream,
                         (bf16*)dx_bf16, da_is_bf16);
}
int64_t rald_op_groupnorm_bwd_scratch_bytes(int32_t B, int32_t S, int32_t C) { return groupnorm_bwd_scratch_bytes(B, S, C); }
int rald_op_groupnorm_apply(const float* x, const double* stats, const float* gamma, const float* beta, void* y_bf16, int32_t B, int32_t S, int32_t C,
                            int32_t swish, void* stream) {
    return groupnorm_apply(x, stats, gamma, beta, (bf16*)y_bf16, B, S, C, swish, (hipStream_t)stream);
}
int rald_op_conv_in(const float* cube, int32_t cube_ch, int32_t Cin, const float* W, const float* bias, float* out, int32_t B, int32_t D, int32_t H,
                    int32_t Wd, int32_t Cout, void* stream) {
    return conv_in_fwd(cube, cube_ch, Cin, W, bias, out, B, D, H, Wd, Cout, (hipStream_t)stream);
}
int rald_op_conv_pack_weights(const float* W, void* out_bf16, int32_t Cout, int32_t Cin, int32_t pad_to, int32_t dgrad, void* stream) {
    return conv_pack_weights(W, (bf16*)out_bf16, Cout, Cin, pad_to, dgrad, (hipStream_t)stream);
}
int rald_op_pad_channels(const float* x, void* out_bf16, int64_t M, int32_t C, int32_t Cpad, void* stream) {
    return pad_channels(x, (bf16*)out_bf16, M, C, Cpad, (hipStream_t)stream);
}
int rald_op_zero_insert2(const float* dy, void* out_bf16, int32_t B, int32_t OD, int32_t OH, int32_t OW, int32_t C, void* stream) {
    return zero_insert2(dy, (bf16*)out_bf16, B, OD, OH, OW, C, (hipStream_t)stream);
}
int rald_op_rowdot(const void* a_bf16, const void* b_bf16, int64_t M, int32_t C, float* out, void* stream) {
    return rowdot((const bf16*)a_bf16, (const bf16*)b_bf16, M, C, out, (hipStream_t)stream);
}
int rald_op_softmax_rows(const float* S, int64_t ld_s, void* P_bf16, int64_t ld_p, int32_t rows, int32_t n, void* stream) {
    RALD_CHECK(S && P_bf16, "rald_op_softmax_rows: null pointer");
    return softmax_rows(S, ld_s, (bf16*)P_bf16, ld_p, rows, n, (hipStream_t)stream);
}
int rald_op_gemm_mx8(const void* A8, const void* scaleA, int64_t lda, int64_t strideA, int64_t strideSA, const void* B8, const void* scaleB,
                     int64_t ldb, int64_t strideB, int64_t strideSB, void* C, int64_t ldc, int64_t strideC, const float* bias, int32_t M,
                     int32_t N, int32_t K, int32_t batch, float alpha, int32_t epilogue, void* stream, int32_t alpha_ncols) {
    RALD_CHECK(A8 && B8 && scaleA && scaleB && C, "rald_op_gemm_mx8: null pointer");
    Mx8Args a;
    a.A8 = (const unsigned char*)A8; a.B8 = (const unsigned char*)B8; a.SA = (const unsigned char*)scaleA; a.SB = (const unsigned char*)scaleB;
    a.strideSA = strideSA; a.strideSB = strideSB;
    GemmArgs& g = a.g;
    g.A = nullptr; g.lda = lda; g.strideA = strideA; g.B = nullptr; g.ldb = ldb; g.strideB = strideB;
    g.C = C; g.ldc = ldc; g.strideC = strideC; g.bias = bias; g.M = M; g.N = N; g.K = K; g.batch = batch; g.alpha = alpha; g.alpha_ncols = alpha_ncols; g.flags = 0;
    return gemm_mx8(a, epilogue, (hipStream_t)stream);
}
int rald_op_gemm_mx8_tile(int32_t M, int32_t N, int32_t batch) { return gemm_mx8_tile(M, N, batch); }
int rald_op_quantize_mx8(const void* in, int32_t in_is_bf16, int64_t ld_in, void* out_e4m3, int64_t ld_out, void* out_scales_e8m0, int64_t rows,
                         int32_t K, void* stream) {
    RALD_CHECK(rows == 0 || (in && out_e4m3 && out_scales_e8m0), "rald_op_quantize_mx8: null pointer");
    return quantize_mx8(in, in_is_bf16, ld_in, (unsigned char*)out_e4m3, ld_out, (unsigned char*)out_scales_e8m0, rows, K, (hipStream_t)stream);
}
int rald_op_layernorm_mx8(const float* x, void* out_e4m3, void* out_scales_e8m0, int64_t M, int32_t D, const float* g, const float* b,
                          int64_t gstride, int32_t rows_per_group, float add_one, float eps, void* stream) {
    RALD_CHECK(M == 0 || (x && out_e4m3 && out_scales_e8m0 && g && b), "rald_op_layernorm_mx8: null pointer");
    return layernorm_mod_mx8(x, (unsigned char*)out_e4m3, (unsigned char*)out_scales_e8m0, M, D, g, b, gstride, rows_per_group, add_one, eps,
                             (hipStream_t)stream);
}
int rald_op_layernorm(const float* x, void* out_bf16, int32_t M, int32_t D, const float* g, const float* b,
                      int64_t gstride, int32_t rows_per_group, float add_one, float eps, void* stream) {
    RALD_CHECK(x && out_bf16 && g && b, "rald_op_layernorm: null pointer");
    return layernorm_mod(x, (bf16*)out_bf16, M, D, g, b, gstride, rows_per_group, add_one, eps, (hipStream_t)stream);
}
int rald_op_attention(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                      const void* Vt, int64_t ldvt, int64_t strideVt, void* O, int64_t ldo, int64_t strideO,
                      int32_t nq, int32_t nk, int32_t k_rows, int32_t heads, int32_t batch, float scale, int32_t q_prescaled, void* stream) {
    RALD_CHECK(Q && K && Vt && O, "rald_op_attention: null pointer");
    AttnArgs a;
    a.Q = (const bf16*)Q; a.ldq = ldq; a.strideQ = strideQ; a.K = (const bf16*)K; a.ldk = ldk; a.strideK = strideK;
    a.Vt = (const bf16*)Vt; a.ldvt = ldvt; a.strideVt = strideVt; a.O = (bf16*)O; a.ldo = ldo; a.strideO = strideO;
    a.nq = nq; a.nk = nk; a.k_rows = k_rows; a.heads = heads; a.batch = batch; a.scale = scale; a.q_prescaled = q_prescaled != 0;
    return attention_d64(a, (hipStream_t)stream);
}
int64_t rald_op_attention_split_scratch_bytes(int32_t ksplit, int32_t nq, int32_t heads, int32_t batch) {
    return attention_split_scratch_bytes(ksplit, nq, heads, batch);
}
int rald_op_attention_split(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, const void* Vt, int64_t ldvt,
                            int64_t strideVt, void* O, int64_t ldo, int64_t strideO, int32_t nq, int32_t nk, int32_t k_rows, int32_t heads,
                            int32_t batch, float scale, int32_t ksplit, void* scratch, void* stream) {
    RALD_CHECK(Q && K && Vt && O, "rald_op_attention_split: null pointer");
    AttnArgs a;
    a.Q = (const bf16*)Q; a.ldq = ldq; a.strideQ = strideQ; a.K = (const bf16*)K; a.ldk = ldk; a.strideK = strideK;
    a.Vt = (const bf16*)Vt; a.ldvt = ldvt; a.strideVt = strideVt; a.O = (bf16*)O; a.ldo = ldo; a.strideO = strideO;
    a.nq = nq; a.nk = nk; a.k_rows = k_rows; a.heads = heads; a.batch = batch; a.scale = scale; a.q_prescaled = 0;
    a.ksplit = ksplit > 0 ? ksplit : attention_pick_ksplit(nq, nk, heads, batch);
    a.part = (float*)scratch;
    return attention_d64(a, (hipStream_t)stream);
}
int rald_op_attention_vrow(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, const void* V, int64_t ldv,
                           int64_t strideV, void* O, int64_t ldo, int64_t strideO, int32_t nq, int32_t nk, int32_t heads, int32_t batch, float scale,
                           void* stream) {
    RALD_CHECK(Q && K && V && O, "rald_op_attention_vrow: null pointer");
    AttnArgs a;
    a.Q = (const bf16*)Q; a.ldq = ldq; a.strideQ = strideQ; a.K = (const bf16*)K; a.ldk = ldk; a.strideK = strideK;
    a.Vt = nullptr; a.ldvt = 0; a.strideVt = 0; a.V = (const bf16*)V; a.ldv = ldv; a.strideV = strideV;
    a.O = (bf16*)O; a.ldo = ldo; a.strideO = strideO;
    a.nq = nq; a.nk = nk; a.k_rows = nk; a.heads = heads; a.batch = batch; a.scale = scale; a.q_prescaled = 0;
    return attention_d64(a, (hipStream_t)stream);
}
int rald_op_attention_bwd(const void* Q, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK, const void* V, int64_t ldv,
                          int64_t strideV, const void* O, int64_t ldo, int64_t strideO, const void* dO, int64_t lddo, int64_t strideDO,
                          void* dQ, int64_t lddq, int64_t strideDQ, void* dK, int64_t lddk, int64_t strideDK, void* dV, int64_t lddv, int64_t strideDV,
                          float* lse_scratch, float* delta_scratch, int32_t nq, int32_t nk, int32_t heads, int32_t batch, float scale, void* stream) {
    AttnBwdArgs a;
    a.Q = (const bf16*)Q; a.ldq = ldq; a.sq = strideQ; a.K = (const bf16*)K; a.ldk = ldk; a.sk = strideK; a.V = (const bf16*)V; a.ldv = ldv; a.sv = strideV;
    a.O = (const bf16*)O; a.ldo = ldo; a.so = strideO; a.dO = (const bf16*)dO; a.lddo = lddo; a.sdo = strideDO;
    a.dQ = (bf16*)dQ; a.lddq = lddq; a.sdq = strideDQ; a.dK = (bf16*)dK; a.lddk = lddk; a.sdk = strideDK; a.dV = (bf16*)dV; a.lddv = lddv; a.sdv = strideDV;
    a.lse = lse_scratch; a.delta = delta_scratch; a.nq = nq; a.nk = nk; a.heads = heads; a.batch = batch; a.scale = scale;
    return attention_bwd_d64(a, (hipStream_t)stream);
}
// fp16 shared-key form (the folded encoder attentions, ae_encode.hip): fp32 pre-scaled queries [batch?][nq][heads*64], ONE fp16 row per key
// [batch][k_rows][64] that is key and value of every head; rows nk .. k_rows-1 must be zero
int rald_op_attention_f16kv(const float* Q, int64_t ldq, int64_t strideQ, const void* KV_f16, void* O_bf16, int64_t ldo, int64_t strideO, int32_t nq,
                            int32_t nk, int32_t k_rows, int32_t heads, int32_t batch, int32_t ksplit, void* scratch, void* stream) {
    RALD_CHECK(Q && KV_f16 && O_bf16, "rald_op_attention_f16kv: null pointer");
    AttnArgs a;
    a.Q = nullptr; a.Qf = Q; a.ldq = ldq; a.strideQ = strideQ; a.f16 = 1;
    a.K = (const bf16*)KV_f16; a.ldk = 64; a.strideK = (int64_t)k_rows * 64;
    a.Vt = nullptr; a.ldvt = 0; a.strideVt = 0; a.V = (const bf16*)KV_f16; a.ldv = 64; a.strideV = (int64_t)k_rows * 64; a.v_padded = 1; a.hsk = 0;
    a.O = (bf16*)O_bf16; a.ldo = ldo; a.strideO = strideO;
    a.nq = nq; a.nk = nk; a.k_rows = k_rows; a.heads = heads; a.batch = batch; a.scale = 1.f; a.q_prescaled = 1;
    a.ksplit = ksplit >= 0 ? ksplit : attention_pick_ksplit(nq, nk, heads, batch);
    a.part = (float*)scratch;
    return attention_d64(a, (hipStream_t)stream);
}
// every field of AttnArgs from the caller (tests): bf16 Q or fp32 Qf, Vt or row-major V, the head stride, the pad contract, the key split
int rald_op_attention_args(const void* Q_bf16, const float* Qf, int64_t ldq, int64_t strideQ, const void* K, int64_t ldk, int64_t strideK,
                           int32_t k_rows, const void* Vt, int64_t ldvt, int64_t strideVt, const void* V, int64_t ldv, int64_t strideV, void* O_bf16,
                           int64_t ldo, int64_t strideO, int32_t nq, int32_t nk, int32_t heads, int32_t batch, float scale, int32_t q_prescaled,
                           int32_t f16, int32_t hsk, int32_t v_padded, int32_t ksplit, void* scratch, int64_t scratch_bytes, void* stream) {
    RALD_CHECK(K && O_bf16 && (Q_bf16 != nullptr) != (Qf != nullptr), "rald_op_attention_args: K, O and one of Q (bf16) and Qf (fp32)");
    RALD_CHECK((Vt != nullptr) != (V != nullptr), "rald_op_attention_args: Vt or a row-major V, not both");
    RALD_CHECK((f16 != 0) == (Qf != nullptr), "rald_op_attention_args: fp32 queries belong to the fp16 form");
    AttnArgs a;
    a.Q = (const bf16*)Q_bf16; a.Qf = Qf; a.ldq = ldq; a.strideQ = strideQ; a.K = (const bf16*)K; a.ldk = ldk; a.strideK = strideK;
    a.Vt = (const bf16*)Vt; a.ldvt = ldvt; a.strideVt = strideVt; a.V = (const bf16*)V; a.ldv = ldv; a.strideV = strideV;
    a.O = (bf16*)O_bf16; a.ldo = ldo; a.strideO = strideO;
    a.nq = nq; a.nk = nk; a.k_rows = k_rows; a.heads = heads; a.batch = batch; a.scale = scale; a.q_prescaled = q_prescaled != 0;
    a.f16 = f16 != 0; a.hsk = hsk; a.v_padded = v_padded != 0;
    RALD_CHECK(nq > 0 && nk > 0 && heads > 0 && batch > 0, "rald_op_attention_args: empty problem");
    a.ksplit = ksplit >= 0 ? ksplit : attention_pick_ksplit(nq, nk, heads, batch);
    a.part = (float*)scratch;
    if (a.ksplit > 1 && a.ksplit <= 64)
        RALD_CHECK(scratch_bytes >= attention_split_scratch_bytes(a.ksplit, nq, heads, batch), "rald_op_attention_args: scratch too small for the key split");
    return attention_d64(a, (hipStream_t)stream);
}
int32_t rald_op_attention_pick_ksplit(int32_t nq, int32_t nk, int32_t heads, int32_t batch) { return attention_pick_ksplit(nq, nk, heads, batch); }
int rald_op_ae_enc_features(const float* pc, const float* basis, const float* var_factor, void* F_f16, void* G_f16, int32_t batch, int32_t n_points,
                            int32_t rows_per_sample, void* stream) {
    RALD_CHECK(pc && basis && var_factor && F_f16 && G_f16, "rald_op_ae_enc_features: null pointer");
    RALD_CHECK(batch >= 1 && n_points >= 1, "rald_op_ae_enc_features: batch and n_points must be at least 1");
    RALD_CHECK(rows_per_sample >= n_points && rows_per_sample % 64 == 0,
               "rald_op_ae_enc_features: rows_per_sample must be a multiple of 64 and at least n_points");
    RALD_CHECK((uintptr_t)F_f16 % 16 == 0 && (uintptr_t)G_f16 % 16 == 0, "rald_op_ae_enc_features: F and G must be 16-byte aligned");
    return ae_enc_features(pc, basis, var_factor, F_f16, G_f16, batch, n_points, rows_per_sample, (hipStream_t)stream);
}
int rald_op_ae_enc_qproj(const float* xin, const float* X0, float* x, const float* gamma, const float* beta, const float* T1, float* Q,
                         int32_t rows, int32_t num_latents, int32_t dim, void* stream) {
    RALD_CHECK(X0 && x && gamma && beta && T1 && Q, "rald_op_ae_enc_qproj: null pointer (only xin may be null)");
    RALD_CHECK(rows >= 1, "rald_op_ae_enc_qproj: rows must be at least 1");
    RALD_CHECK(num_latents >= 1, "rald_op_ae_enc_qproj: num_latents must be at least 1");
    RALD_CHECK(dim == 256 || dim == 512, "rald_op_ae_enc_qproj: dim must be 256 or 512");
    return ae_enc_qproj(xin, X0, x, gamma, beta, T1, Q, rows, num_latents, dim, (hipStream_t)stream);
}
int rald_op_ae_encode_tables(int32_t dim, int32_t num_latents, int32_t heads, int32_t mix, const float* const* in, float* const* out) {
    RALD_CHECK(in && out && dim >= 64 && num_latents >= 1 && heads >= 1, "rald_op_ae_encode_tables: bad argument");
    for (int i = 0; i < 18; ++i) RALD_CHECK(in[i] || (!mix && i >= 2 && i <= 11 && i != 9), "rald_op_ae_encode_tables: null input tensor");
    const int I = heads * 64;
    std::vector<float> Rf, Q1, T4, X0, T1, T3, c3;
    RALD_TRY(rald::ae_encode_tables(dim, I, num_latents, heads, mix != 0, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], in[11],
                                    in[12], in[13], in[14], in[15], in[16], in[17], Rf, Q1, T4, X0, T1, T3, c3));
    const std::vector<float>* v[7] = {&Rf, &Q1, &T4, &X0, &T1, &T3, &c3};
    for (int i = 0; i < 7; ++i)
        if (out[i] && !v[i]->empty()) memcpy(out[i], v[i]->data(), v[i]->size() * 4);
    return 0;
}
int rald_op_proj_in(const float* xin, const float* W, float* x, int32_t M, int32_t C, int32_t D, const float* coef, int32_t coef_stride,
                    int32_t rows_per_group, void* stream) {
    RALD_CHECK(xin && W && x && coef && M >= 1 && rows_per_group >= 1, "rald_op_proj_in: bad argument");
    return proj_in(xin, W, x, M, C, D, coef, coef_stride, rows_per_group, (hipStream_t)stream);
}
int rald_op_final_norm_proj(const float* x, const float* gamma, const float* beta, const float* Wout, const float* xin, float* out, int32_t M,
                            int32_t D, int32_t C, const float* coef, int32_t coef_stride, int32_t rows_per_group, void* stream) {
    RALD_CHECK(x && gamma && beta && Wout && xin && out && coef && M >= 1 && rows_per_group >= 1, "rald_op_final_norm_proj: bad argument");
    return final_norm_proj(x, gamma, beta, Wout, xin, out, M, D, C, coef, coef_stride, rows_per_group, (hipStream_t)stream);
}
int rald_op_attn_self_proj(const void* qkv_bf16, int64_t ld, const void* Wo_bf16, float* part, int32_t n_latents, int32_t heads, int32_t batch,
                           void* stream) {
    return attn_self_proj((const bf16*)qkv_bf16, ld, (const bf16*)Wo_bf16, part, n_latents, heads, batch, (hipStream_t)stream);
}
int rald_op_xattn_q2_proj(const void* h_bf16, const void* Wq_bf16, const void* Kc_bf16, int64_t ldk, int64_t strideK, const void* Vt_bf16,
                          int64_t ldvt, int64_t strideVt, const void* Wo_bf16, float* part, int32_t M, int32_t n_latents, int32_t heads,
                          int32_t n_keys, float qscale, void* stream) {
    return xattn_q2_proj((const bf16*)h_bf16, (const bf16*)Wq_bf16, (const bf16*)Kc_bf16, ldk, strideK, (const bf16*)Vt_bf16, ldvt, strideVt,
                         (const bf16*)Wo_bf16, part, M, n_latents, heads, n_keys, qscale, (hipStream_t)stream);
}
int rald_op_reduce_resid_ln(const float* part, int32_t slabs, int64_t slab_stride, const float* bias, float* x, void* h_bf16, int32_t M,
                            const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps, void* stream) {
    return reduce_resid_ln(part, slabs, slab_stride, bias, x, (bf16*)h_bf16, M, g, b, gstride, rows_per_group, add_one, eps, (hipStream_t)stream);
}
// the three entries above with the slab type as an argument (part_f16 != 0: fp16 slabs of 2^-6 x the value, as dit.hip and ae.hip run them)
int rald_op_attn_self_proj_slabs(const void* qkv_bf16, int64_t ld, const void* Wo_bf16, void* part, int32_t n_latents, int32_t heads, int32_t batch,
                                 int32_t part_f16, void* stream) {
    return attn_self_proj((const bf16*)qkv_bf16, ld, (const bf16*)Wo_bf16, (float*)part, n_latents, heads, batch, (hipStream_t)stream, part_f16 != 0);
}
int rald_op_xattn_q2_proj_slabs(const void* h_bf16, const void* Wq_bf16, const void* Kc_bf16, int64_t ldk, int64_t strideK, const void* Vt_bf16,
                                int64_t ldvt, int64_t strideVt, const void* Wo_bf16, void* part, int32_t M, int32_t n_latents, int32_t heads,
                                int32_t n_keys, float qscale, int32_t part_f16, void* stream) {
    return xattn_q2_proj((const bf16*)h_bf16, (const bf16*)Wq_bf16, (const bf16*)Kc_bf16, ldk, strideK, (const bf16*)Vt_bf16, ldvt, strideVt,
                         (const bf16*)Wo_bf16, (float*)part, M, n_latents, heads, n_keys, qscale, (hipStream_t)stream, part_f16 != 0);
}
int rald_op_reduce_resid_ln_slabs(const void* part, int32_t slabs, int64_t slab_stride, const float* bias, float* x, void* h_bf16, int32_t M,
                                  const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps, int32_t part_f16,
                                  void* stream) {
    RALD_CHECK(part && bias && x && M >= 1 && (!h_bf16 || (g && b && rows_per_group > 0)), "rald_op_reduce_resid_ln_slabs: bad arguments");
    return reduce_resid_ln((const float*)part, slabs, slab_stride, bias, x, (bf16*)h_bf16, M, g, b, gstride, rows_per_group, add_one, eps,
                           (hipStream_t)stream, part_f16 != 0);
}
int rald_op_gemm_resid_ln(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* x, void* h_bf16,
                          const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps,
                          int32_t M, int32_t K, void* stream) {
    GemmLnArgs a;
    a.A = (const bf16*)A; a.lda = lda; a.W = (const bf16*)W; a.ldw = ldw; a.bias = bias; a.x = x; a.h = (bf16*)h_bf16;
    a.g = g; a.b = b; a.gstride = gstride; a.rows_per_group = rows_per_group; a.add_one = add_one; a.eps = eps; a.M = M; a.K = K;
    return gemm_resid_ln(a, (hipStream_t)stream);
}
int rald_op_resid_gemm_ln(const void* A_bf16, const void* A8, const void* SA, int64_t lda, const void* W_bf16, const void* W8, const void* SW,
                          int64_t ldw, int64_t strideW, int32_t w_rows, const float* bias, float* x, void* h_bf16, void* h8, void* hs,
                          const float* g, const float* b, int64_t gstride, int32_t rows_per_group, float add_one, float eps, int32_t M,
                          int32_t K, int32_t nt_io, int32_t route, void* scratch, int64_t scratch_bytes, void* stream) {
    RALD_CHECK(route == 0 || route == 1, "rald_op_resid_gemm_ln: route is 0 (resid_gemm_ln, the product's choice) or 1 (gemm_resid_ln)");
    RALD_CHECK(M > 0 && K > 0 && rows_per_group > 0, "rald_op_resid_gemm_ln: bad shape");
    RALD_CHECK((A_bf16 != nullptr) != (A8 != nullptr), "rald_op_resid_gemm_ln: bf16 operands (A, W) or MXFP8 operands (A8, SA, W8, SW), not both");
    RALD_CHECK(A8 ? (SA && W8 && SW && !W_bf16) : (W_bf16 && !SA && !W8 && !SW), "rald_op_resid_gemm_ln: operand pointers do not match the operand type");
    RALD_CHECK(bias && x && (g != nullptr) == (b != nullptr), "rald_op_resid_gemm_ln: null argument");
    RALD_CHECK(!(h_bf16 && h8) && (h8 != nullptr) == (hs != nullptr), "rald_op_resid_gemm_ln: h or h8 and hs, not both");
    RALD_CHECK(!g || h_bf16 || h8, "rald_op_resid_gemm_ln: a LayerNorm needs h or h8 and hs");
    RALD_CHECK(g || route == 0, "rald_op_resid_gemm_ln: only the dispatcher route runs without a LayerNorm");
    RALD_CHECK((uintptr_t)x % 16 == 0 && (uintptr_t)h_bf16 % 16 == 0 && (uintptr_t)h8 % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)b % 16 == 0 &&
               (uintptr_t)bias % 16 == 0 && gstride % 4 == 0, "rald_op_resid_gemm_ln: 16-byte alignment");
    RALD_CHECK(strideW == 0 || w_rows > 0, "rald_op_resid_gemm_ln: per-group weights need w_rows > 0");
    GemmLnArgs a;
    a.A = (const bf16*)A_bf16; a.lda = lda; a.W = (const bf16*)W_bf16; a.ldw = ldw; a.bias = bias; a.x = x; a.h = (bf16*)h_bf16;
    a.h8 = (unsigned char*)h8; a.hs = (unsigned char*)hs; a.nt_io = nt_io;
    a.A8 = (const unsigned char*)A8; a.SA = (const unsigned char*)SA; a.W8 = (const unsigned char*)W8; a.SW = (const unsigned char*)SW;
    a.g = g; a.b = b; a.gstride = gstride; a.rows_per_group = rows_per_group; a.add_one = add_one; a.eps = eps; a.M = M; a.K = K;
    if (strideW != 0) { a.strideW = strideW; a.w_rows = w_rows; }
    if (route == 1) return gemm_resid_ln(a, (hipStream_t)stream);
    const int splits = splitk_for(M, K);
    if (splits) {
        RALD_CHECK(scratch && (uintptr_t)scratch % 16 == 0, "rald_op_resid_gemm_ln: split-K needs a 16-byte aligned scratch");
        RALD_CHECK(scratch_bytes >= (int64_t)splits * M * 512 * 4, "rald_op_resid_gemm_ln: scratch too small for the split-K slabs");
    }
    // (the unfused route checks its operands in gemm_nt, which knows rows of 8 elements only)
    RALD_CHECK(K % (A8 ? 128 : 64) == 0 && lda % 16 == 0 && ldw % 16 == 0 && lda >= K && ldw >= K, "rald_op_resid_gemm_ln: K and the leading dimensions");
    return resid_gemm_ln(a, 512, (float*)scratch, (hipStream_t)stream);
}
int rald_op_gemm_geglu_mx8out(const void* A_bf16, const void* A8, const void* SA, int64_t lda, const void* W_bf16, const void* W8, const void* SW,
                              int64_t ldw, const float* bias_packed, void* out_bf16, void* out8, void* outs, int64_t ldc, int32_t M, int32_t N,
                              int32_t K, void* stream) {
    RALD_CHECK((A_bf16 != nullptr) != (A8 != nullptr), "rald_op_gemm_geglu_mx8out: bf16 operands (A, W) or MXFP8 operands (A8, SA, W8, SW), not both");
    RALD_CHECK(A8 ? (SA && W8 && SW && !W_bf16) : (W_bf16 && !SA && !W8 && !SW), "rald_op_gemm_geglu_mx8out: operand pointers do not match the operand type");
    RALD_CHECK((out_bf16 != nullptr) != (out8 != nullptr) && (out8 != nullptr) == (outs != nullptr),
               "rald_op_gemm_geglu_mx8out: a bf16 output or out8 and outs, not both");
    RALD_CHECK(bias_packed && M > 0 && N > 0 && K > 0, "rald_op_gemm_geglu_mx8out: null bias or empty problem");
    RALD_CHECK(!out8 || ((uintptr_t)out8 % 16 == 0 && ldc % 32 == 0), "rald_op_gemm_geglu_mx8out: out8 16-byte aligned, ldc a multiple of 32");
    // (with out8 set C is never written; the product passes its bf16 buffer there, the test has none)
    GemmArgs g = gemm_args((const bf16*)A_bf16, lda, (const bf16*)W_bf16, ldw, out_bf16 ? out_bf16 : out8, ldc, bias_packed, M, N, K);
    g.out8 = (unsigned char*)out8; g.outs = (unsigned char*)outs;
    if (!A8) return gemm_nt(g, EPI_GEGLU, (hipStream_t)stream);
    Mx8Args a;
    a.g = g;
    a.A8 = (const unsigned char*)A8; a.SA = (const unsigned char*)SA; a.B8 = (const unsigned char*)W8; a.SB = (const unsigned char*)SW;
    a.strideSA = 0; a.strideSB = 0;
    return gemm_mx8(a, EPI_GEGLU, (hipStream_t)stream);
}
int64_t rald_op_ln_affine_bwd_scratch_bytes(int64_t rows) { return ln_affine_bwd_scratch_bytes(rows); }
int rald_op_ln_affine_bwd(const float* x, const float* dh, const float* gamma, float eps, int64_t rows, float* dx_accum, void* dx_bf16_out,
                          float* dgamma_accum, float* dbeta_accum, void* scratch, int64_t scratch_bytes, void* stream) {
    RALD_CHECK(x && dh && gamma && dx_accum && dgamma_accum && dbeta_accum, "rald_op_ln_affine_bwd: null pointer");
    return ln_affine_bwd(x, dh, gamma, eps, rows, dx_accum, (bf16*)dx_bf16_out, dgamma_accum, dbeta_accum, (float*)scratch, scratch_bytes,
                         (hipStream_t)stream);
}
int64_t rald_op_pe_wgrad_scratch_bytes(int64_t rows) { return pe_wgrad_scratch_bytes(rows); }
int rald_op_pe_wgrad(const float* dY, const float* pts, const float* basis, int64_t rows, float* dW_accum, float* db_accum, void* scratch,
                     int64_t scratch_bytes, void* stream) {
    RALD_CHECK(dY && pts && basis && dW_accum && db_accum, "rald_op_pe_wgrad: null pointer");
    return pe_wgrad(dY, pts, basis, rows, dW_accum, db_accum, (float*)scratch, scratch_bytes, (hipStream_t)stream);
}
int rald_op_point_features(const float* pts, const float* basis, void* feat_bf16, int64_t n, void* stream) {
    RALD_CHECK(pts && basis && feat_bf16, "rald_op_point_features: null pointer");
    return point_features(pts, basis, (bf16*)feat_bf16, n, (hipStream_t)stream);
}
int rald_op_posterior(const float* ml, const float* eps, float* z, float* kl, int32_t B, int32_t rows, int32_t L, void* stream) {
    RALD_CHECK(ml && eps && z && kl && B > 0 && rows > 0 && L > 0, "rald_op_posterior: bad arguments");
    return posterior(ml, eps, nullptr, nullptr, z, kl, B, rows, L, (hipStream_t)stream);
}
int rald_op_posterior_bwd(const float* dz, const float* dkl, const float* ml, const float* eps, float* dml, int32_t B, int32_t rows, int32_t L,
                          void* stream) {
    return posterior_bwd(dz, dkl, ml, eps, dml, B, rows, L, (hipStream_t)stream);
}
int rald_op_scale_rows(const float* in, const float* s, float* x_accum, void* out_bf16, int64_t rows, int32_t cols, int64_t rows_per_sample,
                       void* stream) {
    RALD_CHECK(!x_accum != !out_bf16, "rald_op_scale_rows: exactly one of x_accum / out_bf16");
    return scale_rows(in, s, x_accum, (bf16*)out_bf16, rows, cols, rows_per_sample, (hipStream_t)stream);
}
int rald_op_softmax_bwd_rows(const float* S, const float* dP, const float* delta, int64_t rows, int64_t ld, int32_t n, float scale, void* P_bf16,
                             void* dS_bf16, void* stream) {
    return softmax_bwd_rows(S, dP, delta, rows, ld, n, scale, (bf16*)P_bf16, (bf16*)dS_bf16, (hipStream_t)stream);
}
int64_t rald_op_ae_loss_scratch_bytes(int32_t batch, int64_t n_queries) { return ae_loss_scratch_bytes(batch, n_queries); }
int rald_op_ae_loss(const float* logits, const float* labels, const float* kl, const int32_t* in_voxel_num_dev, int32_t batch, int64_t n_queries,
                    float vol_weight, float near_weight, float kl_weight, float grad_scale, double* out_losses4, int32_t* out_counts3,
                    float* dlogits, float* dkl, void* scratch, int64_t scratch_bytes, void* stream) {
    RALD_CHECK(logits && labels && kl && in_voxel_num_dev && out_losses4 && out_counts3, "rald_op_ae_loss: null pointer");
    return ae_loss(logits, labels, kl, in_voxel_num_dev, batch, n_queries, vol_weight, near_weight, kl_weight, grad_scale, out_losses4, out_counts3,
                   dlogits, dkl, scratch, scratch_bytes, (hipStream_t)stream);
}
int rald_op_cast_bf16(const float* in, void* out_bf16, int64_t n, void* stream) {
    RALD_CHECK(in && out_bf16, "rald_op_cast_bf16: null pointer");
    return cast_f32_bf16(in, (bf16*)out_bf16, n, (hipStream_t)stream);
}

}  // extern "C"
