// real.cpp -- host side of include/fft_wgpu_amd_real.h: plain C++ against the HIP runtime API, no device code.
// Contexts, buffers, streams and the error string are the main library's (../csrc/internal.h, read-only): this library
// links against libfft_wgpu_amd.so and adds the plan object of the real-input transforms.  A plan holds no device memory
// -- the twiddles are compile-time constants of the kernel unit -- so exec allocates nothing and destroy frees nothing on
// the device.
#include "../../include/fft_wgpu_amd_real.h"

#include <new>

#include "../side/side_host.h"
#include "real_kernels.h"

using fwa_int::fail;
using fwa_int::fail_hip;

struct fwr_plan {
    fwa_ctx *ctx = nullptr;
    int32_t kind = 0;
    uint32_t n = 0;
    uint64_t batch = 0, blocks = 0;
    fwa_buf *real = nullptr, *spec = nullptr;  // forward: src, dst; inverse: dst, src
    fwr::Geometry geom;
};

namespace {

// The shape rules create and describe share; *blocks is the grid of one exec.
int32_t check_shape(const fwa_ctx *ctx, uint32_t n, uint64_t batch, fwr::Geometry *g, uint64_t *blocks)
{
    if (!fwa_int::is_pow2(n)) return fail(ctx, FWA_ERR_INVALID_ARG, "fft_len must be a power of two");
    if (n == 1)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "fft_len = 1 has no half-length transform: real plans support fft_len = 2 .. 4096");
    if (n > fwr::MAX_LEN)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "real plans support fft_len = 2 .. 4096, got " + std::to_string(n));
    if (batch > (~0ull) / (4ull * (n + 2))) return fail(ctx, FWA_ERR_INVALID_ARG, "8 * (fft_len / 2 + 1) * batch overflows 64 bits");
    *g = fwr::geometry(n);
    *blocks = fwr::blocks(*g, batch);
    return side::check_grid(ctx, *blocks);
}

}  // namespace

extern "C" {

int32_t fwr_abi_version(void) { return FWR_ABI_VERSION; }

int32_t fwr_describe(uint32_t n, uint64_t batch, int32_t *threads, int32_t *lds_bytes, int32_t *rows_per_block, uint64_t *blocks)
{
    fwr::Geometry g;
    uint64_t b = 0;
    if (int32_t st = check_shape(nullptr, n, batch, &g, &b)) return st;
    if (threads) *threads = g.threads;
    if (lds_bytes) *lds_bytes = g.lds_bytes;
    if (rows_per_block) *rows_per_block = g.rows_per_block;
    if (blocks) *blocks = b;
    return FWA_OK;
}

int32_t fwr_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t n, fwa_buf *src, fwa_buf *dst, fwr_plan **out)
{
    if (!out) return fail(ctx, FWA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx || !src || !dst) return fail(ctx, FWA_ERR_INVALID_ARG, "ctx/src/dst is NULL");
    if (int32_t st = side::check_owner(ctx, src, "src")) return st;
    if (int32_t st = side::check_owner(ctx, dst, "dst")) return st;
    if (int32_t st = side::check_kind(ctx, kind, "real plans")) return st;
    if (side::overlap(src, dst)) return fail(ctx, FWA_ERR_INVALID_ARG, "src and dst overlap: real plans are out of place");
    fwr::Geometry g;
    uint64_t blocks = 0;
    if (int32_t st = check_shape(ctx, n, 0, &g, &blocks)) return st;
    fwa_buf *real = kind == FWA_FORWARD ? src : dst, *spec = kind == FWA_FORWARD ? dst : src;
    const uint64_t real_row = 4ull * n, spec_row = 8ull * (n / 2 + 1);
    if (real->bytes % real_row != 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "the real buffer's size is not a multiple of 4 * fft_len bytes");
    if (spec->bytes % spec_row != 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "the spectrum buffer's size is not a multiple of 8 * (fft_len / 2 + 1) bytes");
    const uint64_t batch = real->bytes / real_row;
    if (spec->bytes / spec_row != batch)
        return fail(ctx, FWA_ERR_INVALID_ARG, "src and dst disagree about batch: " + std::to_string(batch) + " real rows, " +
                    std::to_string(spec->bytes / spec_row) + " spectrum rows");
    if (int32_t st = check_shape(ctx, n, batch, &g, &blocks)) return st;

    USE_DEVICE(ctx);
    if (hipError_t e = fwr::setup_real_kernels(n); e != hipSuccess) return fail_hip(ctx, e, "hipFuncSetAttribute(real kernels)");
    fwr_plan *p = new (std::nothrow) fwr_plan;
    if (!p) return fail(ctx, FWA_ERR_OUT_OF_MEMORY, "host allocation failed");
    p->ctx = ctx; p->kind = kind; p->n = n; p->batch = batch; p->blocks = blocks; p->real = real; p->spec = spec; p->geom = g;
    *out = p;
    return FWA_OK;
}

int32_t fwr_plan_exec(fwr_plan *plan, fwa_stream *stream)
{
    if (!plan) return fail(nullptr, FWA_ERR_INVALID_ARG, "plan is NULL");
    fwa_ctx *ctx = plan->ctx;
    if (int32_t st = side::check_stream(ctx, stream)) return st;
    USE_DEVICE(ctx);
    const int dir = plan->kind == FWA_FORWARD ? fwa::FWD : fwa::INV;
    const float scale = plan->kind == FWA_INVERSE_SCALED ? 1.0f / (float)plan->n : 1.0f;  // an exact power of two
    const hipError_t e = fwr::launch_real(dir, plan->n, static_cast<float *>(plan->real->p), static_cast<float *>(plan->spec->p),
                                          plan->batch, scale, fwa_int::raw(stream));
    if (e != hipSuccess) return fail_hip(ctx, e, "real-plan launch", FWA_ERR_LAUNCH);
    return FWA_OK;
}

int32_t fwr_plan_get_i64(const fwr_plan *plan, const char *key, int64_t *value)
{
    if (int32_t st = side::check_get(plan, key, value)) return st;
    return side::get_i64(plan->ctx, key, value, {
        {"fft_len", (int64_t)plan->n}, {"batch", (int64_t)plan->batch}, {"launches_per_exec", 1},
        {"threads", plan->geom.threads}, {"lds_bytes", plan->geom.lds_bytes}, {"rows_per_block", plan->geom.rows_per_block},
        {"blocks", (int64_t)plan->blocks},
    });
}

int32_t fwr_plan_destroy(fwr_plan *plan)
{
    delete plan;  // nothing on the device belongs to a plan
    return FWA_OK;
}

}  // extern "C"
