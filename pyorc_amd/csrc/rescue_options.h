// The two values the option table (api_core.hip) and the rescue pass (piv_rescue.hip) share.  They live here, and not in
// api_internal.h, because the kernel translation units do not see the host API's header, and not in common.h, because nothing
// that the PIV kernels see changes with them.  Defined in api_core.hip.
#pragma once

#include <atomic>

namespace lspiv_api __attribute__((visibility("hidden"))) {
// "rescue_generic": 1 = the fit kernel with run-time window geometry for every launch (the reference the fixed-size instantiations of
// the square 16 / 32 / 64 px windows are compared against, bit for bit); read by launch_piv_rescue
extern std::atomic<int> g_opt_rescue_generic;
// "rescue_fit_size" (read-only): which instantiation of the fit kernel the last rescue pass of this process launched -- its
// compile-time window size, 0 the run-time-geometry kernel, -1 no pass yet.  Written by launch_piv_rescue; one value for the
// process, so it says something only while one thread launches (the tests of the dispatch conditions).
extern std::atomic<int> g_rescue_fit_size;
}  // namespace lspiv_api
