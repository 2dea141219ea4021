// Host-side helpers of the operator entry points (plain inline functions, no device code): the stream cast, alignment and grid sizes,
// the "who: what" refusal, the dtype and scratch checks, and the f16 / f32 dispatcher that lets an entry point write its launch once.
#pragma once
#include <cstdio>

#include "common.h"
#include "../../include/mebt_hip.h"

namespace {

inline hipStream_t S(mebt_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// 256-thread blocks of a grid-stride kernel over `total` items: at least 1, at most 65536
inline unsigned grid_of(long long total) { const long long g = (total + 255) / 256; return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536); }

// sets the last error to "who: what" and returns `code`
inline int fail(int code, const char* who, const char* what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    mebt_set_error(msg);
    return code;
}

inline int check_dtype(const char* who, int32_t dtype) {
    if (dtype != MEBT_DTYPE_F32 && dtype != MEBT_DTYPE_F16) return fail(MEBT_EDTYPE, who, "dtype must be f32 or f16");
    return MEBT_OK;
}

// a slab of one fp64 (or 64-bit) slot per workgroup: it must hold `need` bytes and start on an 8-byte boundary; the workgroups of one
// launch stay below 2^31
inline int check_scratch(const char* who, const void* scratch, int64_t scratch_bytes, int64_t need, int64_t blocks) {
    if (blocks > 0x7FFFFFFFll) return fail(MEBT_ESHAPE, who, "too large for one launch");
    if (!scratch) return fail(MEBT_EINVAL, who, "null pointer");
    if (reinterpret_cast<uintptr_t>(scratch) & 7) return fail(MEBT_EINVAL, who, "scratch must be 8-byte aligned");
    if (scratch_bytes < need) return fail(MEBT_EWORKSPACE, who, "scratch too small");
    return MEBT_OK;
}

// f(tag) with a value of the element type a checked dtype names: with_dtype(dtype, [&](auto tag) { using T = decltype(tag); ... })
template <typename F>
inline auto with_dtype(int32_t dtype, F&& f) { return dtype == MEBT_DTYPE_F16 ? f(f16_t{}) : f(float{}); }

}  // namespace
