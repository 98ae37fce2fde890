// stft.cpp -- host side of include/fft_wgpu_amd_stft.h: plain C++ against the HIP runtime API, no device code.
// Contexts, buffers, streams and the error string are the main library's (../csrc/internal.h, read-only): this library
// links against libfft_wgpu_amd.so and adds the plan object of the framed real-input transforms.  A plan holds no device
// memory -- the twiddles are compile-time constants of the kernel unit, the window is the caller's buffer -- so exec
// allocates nothing and destroy frees nothing on the device.
#include "../../include/fft_wgpu_amd_stft.h"

#include <new>

#include "../side/side_host.h"
#include "stft_kernels.h"

using fwa_int::fail;
using fwa_int::fail_hip;

struct fwt_plan {
    fwa_ctx *ctx = nullptr;
    int32_t output = 0;
    uint32_t n = 0, hop = 0;
    uint64_t sig_len = 0, signals = 0, per_signal = 0, blocks = 0;
    fwa_buf *src = nullptr, *window = nullptr, *dst = nullptr;
    fwt::Geometry geom;
};

namespace {

// The shape rules create and describe share; *per_signal is F, *blocks the grid of one exec.
int32_t check_shape(const fwa_ctx *ctx, uint32_t n, uint32_t hop, uint64_t L, uint64_t signals, fwt::Geometry *g, uint64_t *per_signal,
                    uint64_t *blocks)
{
    if (!fwa_int::is_pow2(n)) return fail(ctx, FWA_ERR_INVALID_ARG, "fft_len must be a power of two");
    if (n == 1)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "fft_len = 1 has no half-length transform: framed plans support fft_len = 2 .. 4096");
    if (n > fwt::MAX_LEN)
        return fail(ctx, FWA_ERR_UNSUPPORTED, "framed plans support fft_len = 2 .. 4096, got " + std::to_string(n));
    if (hop == 0) return fail(ctx, FWA_ERR_INVALID_ARG, "hop must be at least 1");
    if (L < n)
        return fail(ctx, FWA_ERR_INVALID_ARG, "signal_len " + std::to_string(L) + " is shorter than one frame of fft_len " + std::to_string(n));
    if (L > (~0ull) / 4 || (signals && L > (~0ull) / 4 / signals))
        return fail(ctx, FWA_ERR_INVALID_ARG, "4 * signal_len * signals overflows 64 bits");
    *per_signal = fwt::frames_per_signal(n, hop, L);
    if (signals && *per_signal > (~0ull) / (4ull * (n + 2)) / signals)
        return fail(ctx, FWA_ERR_INVALID_ARG, "8 * (fft_len / 2 + 1) * frames overflows 64 bits");
    *g = fwt::geometry(n);
    *blocks = fwt::blocks(*g, signals * *per_signal);
    return side::check_grid(ctx, *blocks);
}

}  // namespace

extern "C" {

int32_t fwt_abi_version(void) { return FWT_ABI_VERSION; }

int32_t fwt_describe(uint32_t n, uint32_t hop, uint64_t signal_len, uint64_t signals, uint64_t *frames_per_signal, int32_t *threads,
                     int32_t *lds_bytes, int32_t *frames_per_block, uint64_t *blocks)
{
    fwt::Geometry g;
    uint64_t f = 0, b = 0;
    if (int32_t st = check_shape(nullptr, n, hop, signal_len, signals, &g, &f, &b)) return st;
    if (frames_per_signal) *frames_per_signal = f;
    if (threads) *threads = g.threads;
    if (lds_bytes) *lds_bytes = g.lds_bytes;
    if (frames_per_block) *frames_per_block = g.rows_per_block;
    if (blocks) *blocks = b;
    return FWA_OK;
}

int32_t fwt_plan_create(fwa_ctx *ctx, int32_t output, uint32_t n, uint32_t hop, uint64_t signal_len, fwa_buf *src, fwa_buf *window,
                        fwa_buf *dst, fwt_plan **out)
{
    if (!out) return fail(ctx, FWA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx || !src || !dst) return fail(ctx, FWA_ERR_INVALID_ARG, "ctx/src/dst is NULL");
    if (int32_t st = side::check_owner(ctx, src, "src")) return st;
    if (window)
        if (int32_t st = side::check_owner(ctx, window, "window")) return st;
    if (int32_t st = side::check_owner(ctx, dst, "dst")) return st;
    if (output != FWT_SPECTRUM && output != FWT_POWER) return fail(ctx, FWA_ERR_INVALID_ARG, "output is FWT_SPECTRUM or FWT_POWER");
    fwt::Geometry g;
    uint64_t per_signal = 0, blocks = 0;
    if (int32_t st = check_shape(ctx, n, hop, signal_len, 0, &g, &per_signal, &blocks)) return st;
    if (side::overlap(src, dst)) return fail(ctx, FWA_ERR_INVALID_ARG, "src and dst overlap: framed plans are out of place");
    if (window && side::overlap(window, dst)) return fail(ctx, FWA_ERR_INVALID_ARG, "window and dst overlap: the window is never written");
    if (window && window->bytes != 4ull * n)
        return fail(ctx, FWA_ERR_INVALID_ARG, "the window holds " + std::to_string(window->bytes) + " bytes, not 4 * fft_len = " +
                    std::to_string(4ull * n));
    const uint64_t sig_bytes = 4ull * signal_len;
    if (src->bytes % sig_bytes != 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "the size of src is not a multiple of 4 * signal_len bytes");
    const uint64_t signals = src->bytes / sig_bytes;
    if (int32_t st = check_shape(ctx, n, hop, signal_len, signals, &g, &per_signal, &blocks)) return st;
    const uint64_t row = (output == FWT_POWER ? 4ull : 8ull) * (n / 2 + 1), frames = signals * per_signal;
    if (dst->bytes != frames * row)
        return fail(ctx, FWA_ERR_INVALID_ARG, "dst holds " + std::to_string(dst->bytes) + " bytes, not " + std::to_string(frames) +
                    " frames (" + std::to_string(signals) + " signals of " + std::to_string(per_signal) + ") of " + std::to_string(row) + " bytes");

    USE_DEVICE(ctx);
    if (hipError_t e = fwt::setup_stft_kernels(n); e != hipSuccess) return fail_hip(ctx, e, "hipFuncSetAttribute(framed kernels)");
    fwt_plan *p = new (std::nothrow) fwt_plan;
    if (!p) return fail(ctx, FWA_ERR_OUT_OF_MEMORY, "host allocation failed");
    p->ctx = ctx; p->output = output; p->n = n; p->hop = hop; p->sig_len = signal_len; p->signals = signals; p->per_signal = per_signal;
    p->blocks = blocks; p->src = src; p->window = window; p->dst = dst; p->geom = g;
    *out = p;
    return FWA_OK;
}

int32_t fwt_plan_exec(fwt_plan *plan, fwa_stream *stream)
{
    if (!plan) return fail(nullptr, FWA_ERR_INVALID_ARG, "plan is NULL");
    fwa_ctx *ctx = plan->ctx;
    if (int32_t st = side::check_stream(ctx, stream)) return st;
    USE_DEVICE(ctx);
    const hipError_t e = fwt::launch_stft(plan->n, plan->hop, plan->sig_len, plan->signals, plan->output == FWT_POWER,
                                          static_cast<const float *>(plan->src->p),
                                          plan->window ? static_cast<const float *>(plan->window->p) : nullptr,
                                          static_cast<float *>(plan->dst->p), fwa_int::raw(stream));
    if (e != hipSuccess) return fail_hip(ctx, e, "framed-plan launch", FWA_ERR_LAUNCH);
    return FWA_OK;
}

int32_t fwt_plan_get_i64(const fwt_plan *plan, const char *key, int64_t *value)
{
    if (int32_t st = side::check_get(plan, key, value)) return st;
    return side::get_i64(plan->ctx, key, value, {
        {"fft_len", (int64_t)plan->n}, {"hop", (int64_t)plan->hop}, {"signal_len", (int64_t)plan->sig_len},
        {"signals", (int64_t)plan->signals}, {"frames_per_signal", (int64_t)plan->per_signal},
        {"frames", (int64_t)(plan->signals * plan->per_signal)}, {"output", plan->output}, {"windowed", plan->window ? 1 : 0},
        {"launches_per_exec", 1}, {"threads", plan->geom.threads}, {"lds_bytes", plan->geom.lds_bytes},
        {"frames_per_block", plan->geom.rows_per_block}, {"blocks", (int64_t)plan->blocks},
    });
}

int32_t fwt_plan_destroy(fwt_plan *plan)
{
    delete plan;  // nothing on the device belongs to a plan
    return FWA_OK;
}

}  // extern "C"
