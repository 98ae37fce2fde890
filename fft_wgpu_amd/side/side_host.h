// side_host.h -- the host checks that the side plan libraries (../strided, ../fft2d, ../real, ../conv, ../stft) make in the
// same words: stated once, header-only, plain C++ against ../csrc/internal.h like the .cpp files that include it -- no device
// header, no device code.  Status codes and detail strings are behaviour (the tests match words in them).  Everything sits
// in an anonymous namespace: no library exports a symbol of it.  Beside csrc/, not in it: the records stamped with csrc's
// sources do not move when a check here is mended.
#pragma once
#include <cstring>
#include <initializer_list>

#include "../csrc/internal.h"

namespace side {
namespace {

using fwa_int::fail;

// A buffer or stream handed to a plan of `ctx` is one of ctx's own, and ctx is alive (LIVE_HANDLE's rule, with the message on
// the context the caller reads it from).  `name` opens the detail: "the buffer", "src", "the stream", ...
// Every fwa_buf is 16-byte aligned: fwa_buf_alloc hands out allocation bases, fwa_buf_wrap refuses any other pointer.
inline int32_t check_owner(const fwa_ctx *ctx, const fwa_int::Handle *h, const char *name)
{
    if (!h->ctx) return fail(ctx, FWA_ERR_INVALID_ARG, std::string(name) + " belongs to a context that has been destroyed");
    if (h->ctx != ctx) return fail(ctx, FWA_ERR_INVALID_ARG, std::string(name) + " belongs to another context");
    return FWA_OK;
}

// The stream of an exec: NULL (the null stream) or one of the plan's context.
inline int32_t check_stream(const fwa_ctx *ctx, const fwa_stream *stream)
{
    return stream ? check_owner(ctx, stream, "the stream") : FWA_OK;
}

inline bool overlap(const fwa_buf *a, const fwa_buf *b)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a->p), b0 = reinterpret_cast<uintptr_t>(b->p);
    return a0 < b0 + b->bytes && b0 < a0 + a->bytes;
}

// `plans` opens the detail: "strided plans", "2-D plans", "real plans".
inline int32_t check_kind(const fwa_ctx *ctx, int32_t kind, const char *plans)
{
    if (kind == FWA_FORWARD || kind == FWA_INVERSE_SCALED || kind == FWA_INVERSE_UNSCALED) return FWA_OK;
    return fail(ctx, FWA_ERR_INVALID_ARG, std::string(plans) + " are FWA_FORWARD, FWA_INVERSE_SCALED or FWA_INVERSE_UNSCALED");
}

// The grid limit of one launch.  The grid is groups * per_group (per_group >= 1); the product is never formed, so it cannot
// wrap.
inline int32_t check_grid(const fwa_ctx *ctx, uint64_t groups, uint64_t per_group = 1)
{
    if (groups > 0x7fffffffull / per_group)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "the shape needs more than 2^31 - 1 workgroups in one launch");
    return FWA_OK;
}

// *_plan_get_i64 in two steps, since the key list reads the plan: the NULL checks, then the lookup.
template <class Plan>
inline int32_t check_get(const Plan *plan, const char *key, const int64_t *value)
{
    if (!plan || !key || !value) return fail(plan ? plan->ctx : nullptr, FWA_ERR_INVALID_ARG, "plan/key/value is NULL");
    return FWA_OK;
}

struct KeyValue {
    const char *key;
    int64_t v;
};

inline int32_t get_i64(const fwa_ctx *ctx, const char *key, int64_t *value, std::initializer_list<KeyValue> keys)
{
    for (const KeyValue &k : keys)
        if (!std::strcmp(key, k.key)) {
            *value = k.v;
            return FWA_OK;
        }
    return fail(ctx, FWA_ERR_INVALID_ARG, std::string("unknown key: ") + key);
}

}  // namespace
}  // namespace side
