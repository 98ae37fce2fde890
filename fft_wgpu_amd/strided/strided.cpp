// strided.cpp -- host side of include/fft_wgpu_amd_strided.h: plain C++ against the HIP runtime API, no device code.
// Contexts, buffers, streams and the error string are the main library's (../csrc/internal.h, read-only): this library
// links against libfft_wgpu_amd.so and adds the plan object of the strided-batch transforms.  A plan holds no device
// memory -- the twiddles are compile-time constants of the kernel unit -- so exec allocates nothing and destroy frees
// nothing on the device.
#include "../../include/fft_wgpu_amd_strided.h"

#include <new>

#include "../side/side_host.h"
#include "strided_kernels.h"

using fwa_int::fail;
using fwa_int::fail_hip;

struct fws_plan {
    fwa_ctx *ctx = nullptr;
    int32_t kind = 0;
    uint32_t n = 0;
    uint64_t howmany = 0, batch = 0, blocks = 0;
    fwa_buf *buf = nullptr;
    fws::Geometry geom;
};

namespace {

// The shape rules create and describe share; *blocks is the grid of one exec.
int32_t check_shape(const fwa_ctx *ctx, uint32_t fft_len, uint64_t howmany, uint64_t batch, fws::Geometry *g, uint64_t *blocks)
{
    if (!fwa_int::is_pow2(fft_len)) return fail(ctx, FWA_ERR_INVALID_ARG, "fft_len must be a power of two");
    if (fft_len < fws::MIN_LEN || fft_len > fws::MAX_LEN)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "strided plans support fft_len = 2 .. 4096, got " + std::to_string(fft_len));
    if (howmany == 0) return fail(ctx, FWA_ERR_INVALID_ARG, "howmany must be positive");
    if (howmany > (~0ull) / (8ull * fft_len)) return fail(ctx, FWA_ERR_INVALID_ARG, "8 * fft_len * howmany overflows 64 bits");
    *g = fws::geometry(fft_len);
    const uint64_t wgs = fws::wgs_per_matrix(*g, howmany);
    if (int32_t st = side::check_grid(ctx, batch, wgs)) return st;
    *blocks = batch * wgs;
    return FWA_OK;
}

}  // namespace

extern "C" {

int32_t fws_abi_version(void) { return FWS_ABI_VERSION; }

int32_t fws_describe(uint32_t fft_len, uint64_t howmany, uint64_t batch, int32_t *tile_cols, int32_t *threads,
                     int32_t *lds_bytes, uint64_t *blocks)
{
    fws::Geometry g;
    uint64_t b = 0;
    if (int32_t st = check_shape(nullptr, fft_len, howmany, batch, &g, &b)) return st;
    if (tile_cols) *tile_cols = g.tile_cols;
    if (threads) *threads = g.threads;
    if (lds_bytes) *lds_bytes = g.lds_bytes;
    if (blocks) *blocks = b;
    return FWA_OK;
}

int32_t fws_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t fft_len, uint64_t howmany, fwa_buf *buf, fws_plan **out)
{
    if (!out) return fail(ctx, FWA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx || !buf) return fail(ctx, FWA_ERR_INVALID_ARG, "ctx/buf is NULL");
    if (int32_t st = side::check_owner(ctx, buf, "the buffer")) return st;
    if (int32_t st = side::check_kind(ctx, kind, "strided plans")) return st;
    fws::Geometry g;
    uint64_t blocks = 0;
    if (int32_t st = check_shape(ctx, fft_len, howmany, 0, &g, &blocks)) return st;
    const uint64_t mbytes = 8ull * fft_len * howmany;
    if (buf->bytes % mbytes != 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "buffer size is not a multiple of 8 * fft_len * howmany bytes");
    if (int32_t st = check_shape(ctx, fft_len, howmany, buf->bytes / mbytes, &g, &blocks)) return st;
    if (reinterpret_cast<uintptr_t>(buf->p) & 7) return fail(ctx, FWA_ERR_INVALID_ARG, "buffer must be 8-byte aligned");

    USE_DEVICE(ctx);
    if (hipError_t e = fws::setup_strided_kernels(fft_len); e != hipSuccess)
        return fail_hip(ctx, e, "hipFuncSetAttribute(strided kernels)");
    fws_plan *p = new (std::nothrow) fws_plan;
    if (!p) return fail(ctx, FWA_ERR_OUT_OF_MEMORY, "host allocation failed");
    p->ctx = ctx; p->kind = kind; p->n = fft_len; p->howmany = howmany; p->batch = buf->bytes / mbytes;
    p->blocks = blocks; p->buf = buf; p->geom = g;
    *out = p;
    return FWA_OK;
}

int32_t fws_plan_exec(fws_plan *plan, fwa_stream *stream)
{
    if (!plan) return fail(nullptr, FWA_ERR_INVALID_ARG, "plan is NULL");
    fwa_ctx *ctx = plan->ctx;
    if (int32_t st = side::check_stream(ctx, stream)) return st;
    USE_DEVICE(ctx);
    const int dir = plan->kind == FWA_FORWARD ? fwa::FWD : fwa::INV;
    const float scale = plan->kind == FWA_INVERSE_SCALED ? 1.0f / (float)plan->n : 1.0f;  // an exact power of two
    const hipError_t e = fws::launch_strided(dir, plan->n, static_cast<v2f *>(plan->buf->p), plan->howmany, plan->batch,
                                             scale, fwa_int::raw(stream));
    if (e != hipSuccess) return fail_hip(ctx, e, "strided launch", FWA_ERR_LAUNCH);
    return FWA_OK;
}

int32_t fws_plan_get_i64(const fws_plan *plan, const char *key, int64_t *value)
{
    if (int32_t st = side::check_get(plan, key, value)) return st;
    return side::get_i64(plan->ctx, key, value, {
        {"fft_len", (int64_t)plan->n}, {"howmany", (int64_t)plan->howmany}, {"batch", (int64_t)plan->batch},
        {"tile_cols", plan->geom.tile_cols}, {"threads", plan->geom.threads}, {"lds_bytes", plan->geom.lds_bytes},
        {"blocks", (int64_t)plan->blocks}, {"launches_per_exec", 1},
    });
}

int32_t fws_plan_destroy(fws_plan *plan)
{
    delete plan;  // nothing on the device belongs to a plan
    return FWA_OK;
}

}  // extern "C"
