// conv.cpp -- host side of include/fft_wgpu_amd_conv.h: plain C++ against the HIP runtime API, no device code.
// Contexts, buffers, streams and the error string are the main library's (../csrc/internal.h, read-only): this library
// links against libfft_wgpu_amd.so and adds the plan object of the fused FFT-convolution.  A plan holds no device memory
// -- the twiddles are compile-time constants of the kernel unit -- so exec allocates nothing and destroy frees nothing on
// the device.
#include "../../include/fft_wgpu_amd_conv.h"

#include <new>

#include "../side/side_host.h"
#include "conv_kernels.h"

using fwa_int::fail;
using fwa_int::fail_hip;

struct fwc_plan {
    fwa_ctx *ctx = nullptr;
    int32_t kind = 0;
    uint32_t flags = 0, n = 0;
    uint64_t batch = 0, filters = 0, blocks = 0;
    fwa_buf *src = nullptr, *filter = nullptr, *dst = nullptr;
    fwc::Geometry geom;
};

namespace {

// The shape rules create and describe share; *blocks is the grid of one exec.
int32_t check_shape(const fwa_ctx *ctx, uint32_t n, uint64_t batch, fwc::Geometry *g, uint64_t *blocks)
{
    if (!fwa_int::is_pow2(n)) return fail(ctx, FWA_ERR_INVALID_ARG, "fft_len must be a power of two");
    if (n == 1)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "fft_len = 1 is a plain product: convolution plans support fft_len = 2 .. 4096");
    if (n > fwc::MAX_LEN)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "convolution plans support fft_len = 2 .. 4096, got " + std::to_string(n));
    if (batch > (~0ull) / (8ull * n)) return fail(ctx, FWA_ERR_INVALID_ARG, "8 * fft_len * batch overflows 64 bits");
    *g = fwc::geometry(n);
    *blocks = fwc::blocks(*g, batch);
    return side::check_grid(ctx, *blocks);
}

}  // namespace

extern "C" {

int32_t fwc_abi_version(void) { return FWC_ABI_VERSION; }

int32_t fwc_describe(uint32_t n, uint64_t batch, int32_t *threads, int32_t *lds_bytes, int32_t *rows_per_block, uint64_t *blocks)
{
    fwc::Geometry g;
    uint64_t b = 0;
    if (int32_t st = check_shape(nullptr, n, batch, &g, &b)) return st;
    if (threads) *threads = g.threads;
    if (lds_bytes) *lds_bytes = g.lds_bytes;
    if (rows_per_block) *rows_per_block = g.rows_per_block;
    if (blocks) *blocks = b;
    return FWA_OK;
}

int32_t fwc_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t flags, uint32_t n, fwa_buf *src, fwa_buf *filter, fwa_buf *dst,
                        fwc_plan **out)
{
    if (!out) return fail(ctx, FWA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx || !src || !filter || !dst) return fail(ctx, FWA_ERR_INVALID_ARG, "ctx/src/filter/dst is NULL");
    if (int32_t st = side::check_owner(ctx, src, "src")) return st;
    if (int32_t st = side::check_owner(ctx, filter, "filter")) return st;
    if (int32_t st = side::check_owner(ctx, dst, "dst")) return st;
    if (kind != FWA_INVERSE_SCALED && kind != FWA_INVERSE_UNSCALED)
        return fail(ctx, FWA_ERR_INVALID_ARG, "convolution plans are FWA_INVERSE_SCALED or FWA_INVERSE_UNSCALED");
    if (flags & ~(uint32_t)FWC_CONJ_FILTER) return fail(ctx, FWA_ERR_INVALID_ARG, "unknown flag bits: " + std::to_string(flags));
    fwc::Geometry g;
    uint64_t blocks = 0;
    if (int32_t st = check_shape(ctx, n, 0, &g, &blocks)) return st;
    const uint64_t row = 8ull * n;
    if (src->bytes % row != 0 || dst->bytes % row != 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "the size of src / dst is not a multiple of 8 * fft_len bytes");
    if (filter->bytes % row != 0 || filter->bytes == 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "the filter's size is not a positive multiple of 8 * fft_len bytes");
    if (src->bytes != dst->bytes)
        return fail(ctx, FWA_ERR_INVALID_ARG, "src and dst disagree about batch: " + std::to_string(src->bytes / row) + " and " +
                    std::to_string(dst->bytes / row) + " rows");
    if (src != dst && side::overlap(src, dst))
        return fail(ctx, FWA_ERR_INVALID_ARG, "src and dst overlap without being the same buffer: in place means dst == src");
    if (side::overlap(filter, dst)) return fail(ctx, FWA_ERR_INVALID_ARG, "filter and dst overlap: the filter is never written");
    const uint64_t batch = src->bytes / row;
    if (int32_t st = check_shape(ctx, n, batch, &g, &blocks)) return st;

    USE_DEVICE(ctx);
    if (hipError_t e = fwc::setup_conv_kernels(n); e != hipSuccess) return fail_hip(ctx, e, "hipFuncSetAttribute(convolution kernels)");
    fwc_plan *p = new (std::nothrow) fwc_plan;
    if (!p) return fail(ctx, FWA_ERR_OUT_OF_MEMORY, "host allocation failed");
    p->ctx = ctx; p->kind = kind; p->flags = flags; p->n = n; p->batch = batch; p->filters = filter->bytes / row;
    p->blocks = blocks; p->src = src; p->filter = filter; p->dst = dst; p->geom = g;
    *out = p;
    return FWA_OK;
}

int32_t fwc_plan_exec(fwc_plan *plan, fwa_stream *stream)
{
    if (!plan) return fail(nullptr, FWA_ERR_INVALID_ARG, "plan is NULL");
    fwa_ctx *ctx = plan->ctx;
    if (int32_t st = side::check_stream(ctx, stream)) return st;
    USE_DEVICE(ctx);
    const float scale = plan->kind == FWA_INVERSE_SCALED ? 1.0f / (float)plan->n : 1.0f;  // an exact power of two
    const hipError_t e = fwc::launch_conv(plan->n, (plan->flags & FWC_CONJ_FILTER) != 0, static_cast<const v2f *>(plan->src->p),
                                          static_cast<const v2f *>(plan->filter->p), static_cast<v2f *>(plan->dst->p), plan->batch,
                                          plan->filters, scale, fwa_int::raw(stream));
    if (e != hipSuccess) return fail_hip(ctx, e, "convolution-plan launch", FWA_ERR_LAUNCH);
    return FWA_OK;
}

int32_t fwc_plan_get_i64(const fwc_plan *plan, const char *key, int64_t *value)
{
    if (int32_t st = side::check_get(plan, key, value)) return st;
    return side::get_i64(plan->ctx, key, value, {
        {"fft_len", (int64_t)plan->n}, {"batch", (int64_t)plan->batch}, {"filters", (int64_t)plan->filters},
        {"in_place", plan->src == plan->dst ? 1 : 0}, {"launches_per_exec", 1},
        {"threads", plan->geom.threads}, {"lds_bytes", plan->geom.lds_bytes}, {"rows_per_block", plan->geom.rows_per_block},
        {"blocks", (int64_t)plan->blocks},
    });
}

int32_t fwc_plan_destroy(fwc_plan *plan)
{
    delete plan;  // nothing on the device belongs to a plan
    return FWA_OK;
}

}  // extern "C"
