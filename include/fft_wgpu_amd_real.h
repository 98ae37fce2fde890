/*
 * fft_wgpu_amd_real.h -- C ABI of the real-input plans: rfft and irfft of batched rows, out of place, in one launch.
 *
 * With n a power of two and M = n / 2:
 *   FWA_FORWARD            numpy.fft.rfft(x, axis=-1): `src` holds `batch` rows of n f32 back to back, `dst` receives
 *                          `batch` rows of M + 1 samples {f32 re, f32 im} (bins 0 .. n/2) back to back at pitch M + 1 --
 *                          numpy's layout, no padding.
 *   FWA_INVERSE_UNSCALED   n * numpy.fft.irfft(X, n, axis=-1): `src` holds `batch` rows of M + 1 samples, `dst` receives
 *                          `batch` rows of n f32.
 *   FWA_INVERSE_SCALED     numpy.fft.irfft(X, n): the same times 2^-log2 n, exact.
 * As in numpy, the imaginary parts of bin 0 and of bin n/2 of an inverse plan's input take no part in the arithmetic
 * (they are selected away, not multiplied by 0): a NaN or an Inf there does not reach the output.
 *
 * batch = fwa_buf_size(real buffer) / (4 n) and must equal fwa_buf_size(spectrum buffer) / (8 (M + 1)).  Plans are always
 * out of place: `src` is never written, and `src` and `dst` whose byte ranges overlap are refused.  Either buffer may
 * exceed 4 GiB.
 *
 * Built into fft_wgpu_amd/libfft_wgpu_amd_real.so (make -C fft_wgpu_amd/real), which links against libfft_wgpu_amd.so:
 * contexts, buffers, streams, status codes and fwa_last_error_string are those of fft_wgpu_amd.h.  Plain C99; nothing
 * throws or aborts across this boundary.
 *
 * Supported: n = every power of two from 2 to 4096.  What runs (fwr_describe, and the same keys of fwr_plan_get_i64):
 *     n = 2 .. 64       one row per thread, 256 rows per 256-thread workgroup: blocks = ceil(batch / 256)
 *     n = 128 .. 4096   RT adjacent rows per workgroup on the M-point network of the strided-batch plans (threads, LDS
 *                       and RT = tile_cols of fws_describe(M): RT = 16), blocks = ceil(batch / RT)
 *
 * Lifetimes as in fft_wgpu_amd.h: a plan goes before its context, and the buffers outlive the plan.
 */
#ifndef FFT_WGPU_AMD_REAL_H
#define FFT_WGPU_AMD_REAL_H

#include "fft_wgpu_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FWR_ABI_VERSION 1

typedef struct fwr_plan fwr_plan;

int32_t fwr_abi_version(void);

/* Pure host logic, no device: what a plan of length n over `batch` rows launches.  threads, lds_bytes: workgroup size and
 * dynamic LDS; rows_per_block: rows one workgroup owns; blocks = ceil(batch / rows_per_block).  Any output pointer may be
 * NULL.  FWA_ERR_INVALID_ARG: n 0 or not a power of two; FWA_ERR_UNSUPPORTED: n = 1 or n > 4096, or more than 2^31 - 1
 * workgroups.  The detail is read with fwa_last_error_string(NULL). */
int32_t fwr_describe(uint32_t n, uint64_t batch, int32_t *threads, int32_t *lds_bytes, int32_t *rows_per_block,
                     uint64_t *blocks);

/* kind: FWA_FORWARD (src real, dst spectrum), FWA_INVERSE_SCALED or FWA_INVERSE_UNSCALED (src spectrum, dst real).
 * FWA_ERR_INVALID_ARG: a NULL handle, n 0 or not a power of two, FWA_NORMALIZE or an unknown kind, a buffer of another
 * context or of a destroyed one, a buffer size that is not a whole number of rows, buffers that disagree about batch,
 * src and dst whose byte ranges overlap.  FWA_ERR_UNSUPPORTED: as fwr_describe. */
int32_t fwr_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t n, fwa_buf *src, fwa_buf *dst, fwr_plan **out);

/* One launch, asynchronous, stream-ordered on `stream` (a stream of the plan's context; NULL = the null stream),
 * allocates nothing.  FWA_ERR_INVALID_ARG: a NULL plan, a stream of another context or of a destroyed one. */
int32_t fwr_plan_exec(fwr_plan *plan, fwa_stream *stream);

/* Keys: "fft_len", "batch", "launches_per_exec" (always 1), "threads", "lds_bytes", "rows_per_block", "blocks" (what
 * fwr_describe answers). */
int32_t fwr_plan_get_i64(const fwr_plan *plan, const char *key, int64_t *value);

int32_t fwr_plan_destroy(fwr_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FFT_WGPU_AMD_REAL_H */
