// epgx_error.h -- the thread-local message behind epgx_last_error() and the helper that sets it.  Shared by the entry
// points (epgx_api.hip, epgx_signal.hip) and the device-free units behind them (epgx_planner.cpp, epgx_plan_check.cpp,
// epgx_run_check.cpp, epgx_signal_check.cpp); plain C++17.
#pragma once
#include <cstdarg>
#include <cstdio>

namespace epgx {

inline thread_local char g_err[512] = "";

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace epgx
