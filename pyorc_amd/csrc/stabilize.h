// Frame stabilisation (stabilize.hip): the robust transform fit over the vectors of a pair, the chain of poses, the affine warp with one
// matrix per frame (include/lspiv.h, lspiv_stabilize_fit_dev / lspiv_stabilize_chain_dev / lspiv_warp_affine_dev; INTEGRATION.md section
// 2l).  Declarations of its own: nothing here reaches the PIV kernels' headers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lspiv {

struct StabilizeFitParams {
  int rows, cols;          // the window grid of one pair
  double x0, y0;           // centre of window (0, 0) relative to the frame centre: (n - 1) / 2 - (W - 1) / 2, likewise for y
  double dx, dy;           // window pitch n - ox, n - oy
  double cx, cy;           // frame centre (W - 1) / 2, (H - 1) / 2
  int model;               // LSPIV_STABILIZE_TRANSLATION 0, _SIMILARITY 1, _AFFINE 2
  double reject0, reject1;
  int min_vectors;
};

// one block per pair: u, v (pairs, rows, cols) float32 -> P (pairs, 2, 3) float64, n_used (pairs) int32
hipError_t launch_stabilize_fit(const float* u, const float* v, int64_t pairs, const StabilizeFitParams& p, double* P, int32_t* n_used,
                                hipStream_t s);
// one wave: P (pairs, 2, 3), carry_in (2, 3) or NULL (identity) -> A (pairs + 1, 2, 3), carry_out (2, 3) or NULL
hipError_t launch_stabilize_chain(const double* P, int64_t pairs, const double* carry_in, double* A, double* carry_out, hipStream_t s);
// frames (T, H, W) of uint8 (dtype 0) or float32 (dtype 1), A (T, 2, 3) in HBM -> out (T, H, W), another buffer
hipError_t launch_warp_affine(const void* frames, int dtype, int64_t T, int H, int W, const double* A, void* out, hipStream_t s);

}  // namespace lspiv
