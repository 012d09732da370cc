// Pyramidal Lucas-Kanade point tracking (track.hip): the Gaussian pyramid and the tracker of one (point, pair) per wave
// (include/lspiv.h, lspiv_pyr_down[_dev] / lspiv_lk_track[_dev]).  Declarations of its own: nothing here
// reaches the PIV kernels' headers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lspiv {

constexpr int kTrackMaxLevels = 5;
constexpr int kTrackMinWindow = 5, kTrackMaxWindow = 31;   // odd
constexpr int kTrackMaxIter = 100;

// One launch: n_pairs pairs of N points.  Every pointer is already moved to the launch's first pair (frames, pyramid levels, points,
// guess, outputs), so that a batch of a longer run is the same launch on other pointers.
struct LkParams {
  const void* frames;                        // level 0: frames (n_pairs + 1, H[0], W[0]) of the stack's own type
  const float* pyr[kTrackMaxLevels];         // level l >= 1: (n_pairs + 1, H[l], W[l]) float32; [0] unused
  int H[kTrackMaxLevels], W[kTrackMaxLevels];
  int64_t n_pairs;
  int N;
  const double* points;  int64_t points_stride;   // (x, y) per point; doubles from one pair's points to the next (0: the same for all)
  const double* guess;   int64_t guess_stride;    // NULL: start at 0
  int levels, max_iter;
  double eps2, min_eig;
  double *u, *v, *err, *lam;                 // (n_pairs, N)
  int32_t* n_iter;
  uint8_t* status;
  double* next;                              // NULL, or (n_pairs, N, 2): point + (u, v) -- the next row of a trajectory
};

// frames (T, H, W) of uint8 (dtype 0) or float32 (dtype 1) -> out (T, (H + 1) / 2, (W + 1) / 2) float32
hipError_t launch_pyr_down(const void* frames, int dtype, int64_t T, int H, int W, float* out, hipStream_t s);
// window: odd, kTrackMinWindow .. kTrackMaxWindow
hipError_t launch_lk_track(const LkParams& p, int dtype, int window, hipStream_t s);

}  // namespace lspiv
