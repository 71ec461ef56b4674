// LiDAR front end: raw scans -> cropped cartesian points -> voxels -> occupancy queries (lidar.hip).
//
// Frames have different point counts: they travel packed, [total][F] float32, with host int64 offsets [B + 1].  Every output of a
// frame is a function of that frame alone (no float atomics; integer counters only order-free counts), so a frame's result is
// bit-identical in any batch and from run to run.
#pragma once
#include <string>

#include "common.h"
#include "../../include/rald_hip.h"

namespace rald {

struct Lidar {
    rald_lidar_config cfg;
    int64_t grid[3];          // round((hi - lo) / v) per axis
    int64_t cells;            // grid[0] * grid[1] * grid[2] (< 2^31)
    int key_passes;           // 8-bit LSD passes that cover the keys 0 .. cells (cells = the out-of-grid sentinel)
};

int lidar_check_config(const rald_lidar_config& cfg, Lidar* out);
int64_t lidar_workspace_bytes(const Lidar& h, int32_t batch, int64_t total_points);
int lidar_crop(const Lidar& h, const float* points, int32_t in_stride, const int64_t* offsets, int32_t batch, float* out, int32_t* counts,
               void* workspace, int64_t workspace_bytes, hipStream_t st);
int lidar_voxelize(const Lidar& h, const float* points, const int64_t* offsets, const int32_t* counts, int32_t batch, int32_t to_polar,
                   float* polar_out, float* voxels, int32_t* coords, int32_t* num_points, int32_t* kept_keys, int32_t* voxel_counts,
                   void* workspace, int64_t workspace_bytes, hipStream_t st);
int lidar_queries(const Lidar& h, const float* points, const int64_t* offsets, int32_t batch, int32_t num_samples, int32_t in_num,
                  const int64_t* sample_idx, const double* u_in, const int64_t* voxel_idx, const double* u_out, const int64_t* empty_rank,
                  const int32_t* coords, const int32_t* kept_keys, const int32_t* voxel_counts, float* lidar_points, float* query_points,
                  float* query_labels, void* workspace, int64_t workspace_bytes, hipStream_t st);

}  // namespace rald
