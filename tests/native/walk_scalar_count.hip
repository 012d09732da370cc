// Compile-only: the flagship 32 x 32 walking kernel (uint8, no planes, no signal score, batched fit, un-packing through DPP, lane-swap
// reductions) in its former form and with the scalar epilogue, in a translation unit that holds nothing else
// (tests/test_walk_scalar_epilogue_host.py).
#include "piv_fft_impl.h"

template __global__ void lspiv::piv_fft_walk_kernel<uint8_t, 32, false, false, true, true, true, false>(lspiv::PivParams);
template __global__ void lspiv::piv_fft_walk_kernel<uint8_t, 32, false, false, true, true, true, true>(lspiv::PivParams);
