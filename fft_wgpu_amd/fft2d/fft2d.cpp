// fft2d.cpp -- host side of include/fft_wgpu_amd_2d.h: plain C++ against the HIP runtime API, no device code.
// Contexts, buffers, streams and the error string are the main library's (../csrc/internal.h, read-only); the column pass
// is a strided-batch plan, created, run and destroyed through the public fws_* calls.  A plan holds no device memory, so
// exec allocates nothing and destroy frees nothing on the device.
#include "../../include/fft_wgpu_amd_2d.h"

#include <new>

#include "../side/side_host.h"
#include "fft2d_kernels.h"

using fwa_int::fail;
using fwa_int::fail_hip;

struct fw2_plan {
    fwa_ctx *ctx = nullptr;
    int32_t kind = 0;
    uint32_t rows = 0, cols = 0;
    uint64_t batch = 0, row_blocks = 0, col_blocks = 0;
    fwa_buf *buf = nullptr;
    fws_plan *columns = nullptr;  // the second launch; NULL on the fused path
    fw2::Geometry geom;
};

namespace {

int32_t check_axis(const fwa_ctx *ctx, const char *name, uint32_t n)
{
    if (!fwa_int::is_pow2(n)) return fail(ctx, FWA_ERR_INVALID_ARG, std::string(name) + " must be a power of two");
    if (n == 1)
        return fail(ctx, FWA_ERR_UNSUPPORTED, std::string(name) + " = 1 is a 1-D transform: use the 1-D plans (fwa_plan over the "
                    "rows, fws_plan over the columns); 2-D plans support 2 .. 4096");
    if (n > fw2::MAX_LEN)
        return fail(ctx, FWA_ERR_UNSUPPORTED, std::string("2-D plans support ") + name + " = 2 .. 4096, got " + std::to_string(n));
    return FWA_OK;
}

// The shape rules create and describe share; *row_blocks is the grid of the row launch.
int32_t check_shape(const fwa_ctx *ctx, uint32_t rows, uint32_t cols, uint64_t batch, fw2::Geometry *g, uint64_t *row_blocks)
{
    if (int32_t st = check_axis(ctx, "rows", rows)) return st;
    if (int32_t st = check_axis(ctx, "cols", cols)) return st;
    if (batch > (~0ull) / (8ull * rows * cols)) return fail(ctx, FWA_ERR_INVALID_ARG, "8 * rows * cols * batch overflows 64 bits");
    *g = fw2::geometry(rows, cols);
    *row_blocks = fw2::row_blocks(*g, batch * rows, cols);
    return side::check_grid(ctx, *row_blocks);
}

}  // namespace

extern "C" {

int32_t fw2_abi_version(void) { return FW2_ABI_VERSION; }

int32_t fw2_describe(uint32_t rows, uint32_t cols, uint64_t batch, int32_t *launches, int32_t *row_threads,
                     int32_t *row_lds_bytes, uint64_t *row_blocks)
{
    fw2::Geometry g;
    uint64_t b = 0;
    if (int32_t st = check_shape(nullptr, rows, cols, batch, &g, &b)) return st;
    if (!g.fused)  // the column launch has a grid limit of its own
        if (int32_t st = fws_describe(rows, cols, batch, nullptr, nullptr, nullptr, nullptr)) return st;
    if (launches) *launches = g.launches;
    if (row_threads) *row_threads = g.row_threads;
    if (row_lds_bytes) *row_lds_bytes = g.row_lds_bytes;
    if (row_blocks) *row_blocks = b;
    return FWA_OK;
}

int32_t fw2_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t rows, uint32_t cols, fwa_buf *buf, fw2_plan **out)
{
    if (!out) return fail(ctx, FWA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx || !buf) return fail(ctx, FWA_ERR_INVALID_ARG, "ctx/buf is NULL");
    if (int32_t st = side::check_owner(ctx, buf, "the buffer")) return st;
    if (int32_t st = side::check_kind(ctx, kind, "2-D plans")) return st;
    fw2::Geometry g;
    uint64_t blocks = 0;
    if (int32_t st = check_shape(ctx, rows, cols, 0, &g, &blocks)) return st;
    const uint64_t ibytes = 8ull * rows * cols;
    if (buf->bytes % ibytes != 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "buffer size is not a multiple of 8 * rows * cols bytes");
    const uint64_t batch = buf->bytes / ibytes;
    if (int32_t st = check_shape(ctx, rows, cols, batch, &g, &blocks)) return st;
    if (reinterpret_cast<uintptr_t>(buf->p) & 15) return fail(ctx, FWA_ERR_INVALID_ARG, "buffer must be 16-byte aligned");

    USE_DEVICE(ctx);
    if (hipError_t e = fw2::setup_fft2d_kernels(rows, cols); e != hipSuccess)
        return fail_hip(ctx, e, "hipFuncSetAttribute(2-D row kernels)");
    fw2_plan *p = new (std::nothrow) fw2_plan;
    if (!p) return fail(ctx, FWA_ERR_OUT_OF_MEMORY, "host allocation failed");
    p->ctx = ctx; p->kind = kind; p->rows = rows; p->cols = cols; p->batch = batch; p->row_blocks = blocks; p->buf = buf;
    p->geom = g;
    if (!g.fused) {
        int64_t col_blocks = 0;
        int32_t st = fws_plan_create(ctx, kind, rows, cols, buf, &p->columns);  // the detail is already on the context
        if (st == FWA_OK) st = fws_plan_get_i64(p->columns, "blocks", &col_blocks);
        if (st != FWA_OK) {
            fw2_plan_destroy(p);
            return st;
        }
        p->col_blocks = (uint64_t)col_blocks;
    }
    *out = p;
    return FWA_OK;
}

int32_t fw2_plan_exec(fw2_plan *plan, fwa_stream *stream)
{
    if (!plan) return fail(nullptr, FWA_ERR_INVALID_ARG, "plan is NULL");
    fwa_ctx *ctx = plan->ctx;
    if (int32_t st = side::check_stream(ctx, stream)) return st;
    USE_DEVICE(ctx);
    const int dir = plan->kind == FWA_FORWARD ? fwa::FWD : fwa::INV;
    const bool scaled = plan->kind == FWA_INVERSE_SCALED;  // 1 / cols here, 1 / rows in the column pass: exact powers of two
    const float row_scale = scaled ? 1.0f / (float)plan->cols : 1.0f, col_scale = scaled ? 1.0f / (float)plan->rows : 1.0f;
    const hipError_t e = fw2::launch_fft2d_rows(dir, plan->rows, plan->cols, static_cast<v2f *>(plan->buf->p), plan->batch,
                                                row_scale, col_scale, fwa_int::raw(stream));
    if (e != hipSuccess) return fail_hip(ctx, e, "2-D row launch", FWA_ERR_LAUNCH);
    return plan->columns ? fws_plan_exec(plan->columns, stream) : FWA_OK;
}

int32_t fw2_plan_get_i64(const fw2_plan *plan, const char *key, int64_t *value)
{
    if (int32_t st = side::check_get(plan, key, value)) return st;
    return side::get_i64(plan->ctx, key, value, {
        {"rows", (int64_t)plan->rows}, {"cols", (int64_t)plan->cols}, {"batch", (int64_t)plan->batch},
        {"launches_per_exec", plan->geom.launches}, {"row_threads", plan->geom.row_threads},
        {"row_lds_bytes", plan->geom.row_lds_bytes}, {"row_blocks", (int64_t)plan->row_blocks},
        {"col_blocks", (int64_t)plan->col_blocks},
    });
}

int32_t fw2_plan_destroy(fw2_plan *plan)
{
    if (plan) fws_plan_destroy(plan->columns);
    delete plan;  // nothing on the device belongs to a plan
    return FWA_OK;
}

}  // extern "C"
