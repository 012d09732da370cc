// Vector validation on the result block (validate.hip): the normalised median test over the 3 x 3 neighbourhood, with the runner-up
// vector of the second correlation peak as the first substitute.  Declarations of its own: nothing here reaches the PIV kernels' headers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lspiv {

struct ValidateParams {
  float threshold, epsilon;
  int min_neighbours;
  int replace;   // LSPIV_VALIDATE_NAN 0, LSPIV_VALIDATE_MEDIAN 1
};

// ONE Jacobi iteration over (T, R, C): (u_in, v_in) -> (u_out, v_out), which must be other buffers (a lane reads its neighbours'
// inputs); flag is read and written by its own lane only, one buffer serves both (`first`: the incoming flags count as 0).
// peak2: (T, R, C, 4) = {u2, v2, corr2, ratio} or NULL.
hipError_t launch_validate(const float* u_in, const float* v_in, const float* peak2, int64_t T, int R, int C, const ValidateParams& p,
                           bool first, float* u_out, float* v_out, uint8_t* flag, hipStream_t s);

}  // namespace lspiv
