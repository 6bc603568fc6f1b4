// common.h -- shared helpers of libampnet_hip.so (gfx950 only; wavefront = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include "../../include/ampnet_hip.h"

namespace ampnet {

constexpr int WAVE = 64;

// thread-local error text returned by ampnet_last_error()
char *err_buf();
int fail(int code, const char *fmt, ...);

inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return AMPNET_OK;
}

// Raises the dynamic-LDS limit of kernel KERN above the 64 KB default, once per kernel instantiation; `who` opens the error text.
template <auto KERN>
int allow_dynamic_lds(size_t lds, const char *who)
{
    static bool done = false;
    if (done) return AMPNET_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "%s: hipFuncSetAttribute(%zu B LDS): %s", who, lds, hipGetErrorString(e));
    done = true;
    return AMPNET_OK;
}

#define AMPNET_REQUIRE(cond, ...)                                   \
    do {                                                            \
        if (!(cond)) return ::ampnet::fail(AMPNET_E_ARG, __VA_ARGS__); \
    } while (0)
// a step that returns AMPNET_OK or a failure's code (ampnet_last_error already set): the failure is the caller's result
#define AMPNET_TRY(...)                                             \
    do {                                                            \
        const int try_rc_ = (__VA_ARGS__);                          \
        if (try_rc_ != AMPNET_OK) return try_rc_;                   \
    } while (0)

// Optional per-kernel timing with HIP events on the launch stream (bench.py's roofline leg): off by default,
// when on every instrumented launch is bracketed by two events; ampnet_profile_read() synchronises and sums.
struct ProfScope {
    ProfScope(const char *name, double flops, double bytes, hipStream_t st);
    ~ProfScope();
    int slot;
    hipStream_t st;
};

// MFMA operand precision a dispatch on this thread sees: the top of the thread's scope stack (ampnet_precision_scope_begin), else the
// process-wide default (ampnet_set_matrix_precision)
int matrix_precision();

// forward-workspace precision tags (core.hip): set by a train-mode forward, checked by its backward
void ws_tag_set(const void *ws, int mode);
int ws_tag_check(const void *ws, const char *who);

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace ampnet
