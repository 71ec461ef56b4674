// Radar front end: raw ADC frames -> RAEIVV cubes (radar_dsp.hip).  The host tables are built once, in double, at create.
#pragma once
#include <string>
#include <vector>

#include "common.h"
#include "../../include/rald_hip.h"

namespace rald {

struct RadarDsp {
    rald_radar_dsp_config cfg;
    int nch = 0;                      // ntx * nrx data channels
    int nc_used = 0, ns_used = 0;     // chirps / samples the Doppler / range FFTs read (numpy crops n < length)
    int crop_lo = 0, crop_hi = 0;     // zeroed range bins at the head / tail
    int nel = 0, naz = 0;             // dense virtual grid the angle DFT reads (truncated to the FFT sizes like numpy's n < length)
    int npairs = 0;                   // (channel, grid cell) contributions, in the reference's loop order
    // device tables (one allocation): range window [ns], FFT twiddles exp(-2 pi i k / 256) [128], velocity compensation [ntx][nd],
    // azimuth / elevation DFT rows with the fftshift folded in [A][naz] / [E][nel], velocity of each Doppler bin [nd],
    // pair list int2 {channel, cell} [npairs]
    void* dev = nullptr;
    const float* win = nullptr;
    const float2* tw = nullptr;
    const float2* vcomp = nullptr;
    const float2* waz = nullptr;
    const float2* wel = nullptr;
    const float* vbins = nullptr;
    const int2* pairs = nullptr;

    ~RadarDsp();
};

// Sizes and crops only (what the workspace query needs)
int radar_dsp_check_sizes(const rald_radar_dsp_config& cfg);
// Validation and host tables only (no device call): fills everything but the device pointers.
int radar_dsp_plan(const rald_radar_dsp_config& cfg, const int32_t* tx, const int32_t* rx, const double* vbins, int32_t n_vbins, RadarDsp& h,
                   std::vector<char>* tables);
int64_t radar_dsp_workspace_bytes(const rald_radar_dsp_config& cfg, int32_t batch);
int radar_dsp_create(const rald_radar_dsp_config& cfg, const int32_t* tx, const int32_t* rx, const double* vbins, int32_t n_vbins,
                     RadarDsp** out);
// frames: int16 [B][ntx][nrx][nc][ns][2] (input_kind 0) or fp32 [B][ntx][nrx][nc][ns][2] without mean removal (input_kind 1)
int radar_dsp_run(const RadarDsp& h, const void* frames, int input_kind, int32_t batch, float* out, void* workspace, int64_t workspace_bytes,
                  hipStream_t st);

}  // namespace rald
