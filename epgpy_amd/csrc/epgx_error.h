// epgx_error.h -- the thread-local message behind epgx_last_error() and the helper that sets it.  Shared by the entry
// points (epgx_api.hip) and the launch planner (epgx_planner.cpp); plain C++17.
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
