// Helper-point extraction: RAEIVV intensity cubes -> CFAR query points (radar_points.hip).  The host tables (interpolation
// indices and weights, float32 coordinate axes, keep masks) are built once at create.
//
// Tie rule (this project's contract; the reference's np.argpartition / np.argsort leave it undefined): within a range slice the
// chosen points are the k largest values, and among equal values the lowest flat index a * tgt_e + e wins.  The points of a slice
// come out by value descending, equal values by flat index ascending; slices come out in ascending range order.
#pragma once
#include <string>
#include <vector>

#include "common.h"
#include "../../include/rald_hip.h"

namespace rald {

// one target index along one axis of F.interpolate(mode='trilinear', align_corners=False): value = x[i0] * w0 + x[i1] * w1
struct PtsLerp {
    int i0, i1;
    float w0, w1;
};

struct RadarPoints {
    rald_radar_points_config cfg;
    // device tables (one allocation): lerp r [tgt_r] | lerp a [tgt_a] | lerp e [tgt_e] | axis r / a / e float32 | keep r / a / e uint8
    void* dev = nullptr;
    const PtsLerp* lr = nullptr;
    const PtsLerp* la = nullptr;
    const PtsLerp* le = nullptr;
    const float* ax_r = nullptr;
    const float* ax_a = nullptr;
    const float* ax_e = nullptr;
    const uint8_t* keep_r = nullptr;
    const uint8_t* keep_a = nullptr;
    const uint8_t* keep_e = nullptr;

    ~RadarPoints();
};

// Sizes only (what the workspace query needs)
int radar_points_check_config(const rald_radar_points_config& cfg);
int64_t radar_points_workspace_bytes(const rald_radar_points_config& cfg, int32_t batch);
int radar_points_create(const rald_radar_points_config& cfg, const float* axis_r, const float* axis_a, const float* axis_e,
                        const uint8_t* keep_r, const uint8_t* keep_a, const uint8_t* keep_e, RadarPoints** out);
// cubes fp32 [B][in_r][in_a][in_e][in_channels] (channel 0 read); see rald_radar_points_run for the outputs
int radar_points_run(const RadarPoints& h, const float* cubes, int32_t batch, float* points, int32_t* counts, int32_t* peaks, float* intensities,
                     void* workspace, int64_t workspace_bytes, hipStream_t st);

}  // namespace rald
