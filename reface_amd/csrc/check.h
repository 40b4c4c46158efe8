// Argument checks of the C-ABI entry points: no HIP include, so that host-only cores (gemm_plan.h) and their host programs under
// tests/ can use them.  rf::set_error is norm.hip's in the library (behind rf_last_error); a host program brings its own.
#pragma once

namespace rf {

void set_error(const char* fmt, ...);

#define RF_CHECK(cond, ...)                                     \
    do {                                                        \
        if (!(cond)) {                                          \
            rf::set_error(__VA_ARGS__);                         \
            return 1;                                           \
        }                                                       \
    } while (0)

}  // namespace rf
