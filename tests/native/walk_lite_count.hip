// Compile-only: the flagship 32 x 32 walking kernel (uint8, no planes, no signal score, batched fit, un-packing through DPP) in its
// former form and in its "lds_light" form, in a translation unit that holds nothing else (tests/test_walk_lds_light_host.py).
#include "piv_fft_impl.h"

template __global__ void lspiv::piv_fft_walk_kernel<uint8_t, 32, false, false, true, true, false>(lspiv::PivParams);
template __global__ void lspiv::piv_fft_walk_kernel<uint8_t, 32, false, false, true, true, true>(lspiv::PivParams);
