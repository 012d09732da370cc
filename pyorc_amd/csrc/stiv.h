// Space-time image velocimetry (stiv.hip): the gather of the space-time images along the search lines and the orientation of their
// streaks by the structure tensor (include/lspiv.h, lspiv_sti_gather_dev / lspiv_sti_orientation_dev).
// Declarations of its own: nothing here reaches the PIV kernels' headers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lspiv {

constexpr int kStiMaxSmooth = 3;   // passes of the 3 x 3 binomial before the Sobel pair: the stencil is (2k + 3) x (2k + 3)

// The sample table of one call, three arrays of n_points = S * L entries in HBM: the element offset iy * W + ix of the upper left
// neighbour inside a frame and the float32 fractions fx, fy.  Prepared once per call on the host (api_stiv.hip, sti_prepare_points).
struct StiTable {
  const int32_t* offset;
  const float* fx;
  const float* fy;
};
inline size_t sti_table_bytes(int64_t n_points) { return (size_t)n_points * (sizeof(int32_t) + 2 * sizeof(float)); }

// frames (T, H, W) of uint8 (dtype 0) or float32 (dtype 1) -> rows [t_offset, t_offset + T) of sti (S, T_total, L) float32
hipError_t launch_sti_gather(const void* frames, int dtype, int64_t T, int H, int W, const StiTable& table, int64_t S, int L, float* sti,
                             int64_t t_offset, int64_t T_total, hipStream_t s);
// sti (S, T, L) float32 -> tensor (S, K, 3) = (Jxx, Jtt, Jxt), slope (S, K), coherency (S, K), all float64; K windows of Tw rows from
// row k * stride on; smooth 0 .. kStiMaxSmooth
hipError_t launch_sti_orientation(const float* sti, int64_t S, int64_t T, int L, int64_t Tw, int64_t stride, int64_t K, int smooth, bool detrend,
                                  double* tensor, double* slope, double* coherency, hipStream_t s);

}  // namespace lspiv
