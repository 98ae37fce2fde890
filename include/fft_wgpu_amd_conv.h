/*
 * fft_wgpu_amd_conv.h -- C ABI of the fused FFT-convolution plans: ifft(fft(x) * H) of batched rows in one launch.
 *
 * With n a power of two from 2 to 4096: `src` and `dst` each hold `batch` rows of n samples {f32 re, f32 im} back to back;
 * `filter` holds F >= 1 rows of n samples, each a filter SPECTRUM in natural bin order -- exactly what an FWA_FORWARD plan
 * of length n writes.  Row b uses filter row b mod F: a (B, C, n) signal with a (C, n) filter bank is F = C; F need not
 * divide batch.
 *   FWA_INVERSE_SCALED     dst[b] = numpy.fft.ifft(numpy.fft.fft(src[b]) * filter[b % F]): circular convolution.  The
 *                          1 / n is 2^-log2 n, exact, fused into the store.
 *   FWA_INVERSE_UNSCALED   n times that.
 *   flags & FWC_CONJ_FILTER   multiply by conj(filter) instead: circular cross-correlation.  The filter is conjugated on
 *                          use, at no extra pass.
 *
 * batch = fwa_buf_size(src) / (8 n) = fwa_buf_size(dst) / (8 n), F = fwa_buf_size(filter) / (8 n).  `dst` may be `src`
 * (the same buffer handle): the in-place form.  `src` and `dst` that overlap in any other way are refused, and so is a
 * `filter` that overlaps `dst`.  `filter` and, out of place, `src` are never written.  Any of the three buffers may exceed
 * 4 GiB.  The kernels move 16 bytes per access for n <= 32 and rely on what every fwa_buf guarantees: a 16-byte aligned
 * start (fwa_buf_alloc hands out allocation bases, fwa_buf_wrap refuses any other pointer); there is no check of its own.
 *
 * Built into fft_wgpu_amd/libfft_wgpu_amd_conv.so (make -C fft_wgpu_amd/conv), which links against libfft_wgpu_amd.so:
 * contexts, buffers, streams, status codes and fwa_last_error_string are those of fft_wgpu_amd.h.  Plain C99; nothing
 * throws or aborts across this boundary.
 *
 * What runs (fwc_describe, and the same keys of fwc_plan_get_i64):
 *     n = 2 .. 32       one 256-thread workgroup per 64-KiB chunk = 8192 / n rows: blocks = ceil(batch * n / 8192)
 *     n = 64 .. 4096    RT adjacent rows per workgroup on the n-point network of the strided-batch plans (threads, LDS
 *                       and RT = tile_cols of fws_describe(n): 16, 8 at 4096), blocks = ceil(batch / RT)
 *
 * Lifetimes as in fft_wgpu_amd.h: a plan goes before its context, and the buffers outlive the plan.
 */
#ifndef FFT_WGPU_AMD_CONV_H
#define FFT_WGPU_AMD_CONV_H

#include "fft_wgpu_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FWC_ABI_VERSION 1

#define FWC_CONJ_FILTER 1u /* multiply by conj(filter): circular cross-correlation */

typedef struct fwc_plan fwc_plan;

int32_t fwc_abi_version(void);

/* Pure host logic, no device: what a plan of length n over `batch` rows launches.  threads, lds_bytes: workgroup size and
 * dynamic LDS; rows_per_block: rows one workgroup owns; blocks = ceil(batch / rows_per_block).  Any output pointer may be
 * NULL.  FWA_ERR_INVALID_ARG: n 0 or not a power of two; FWA_ERR_UNSUPPORTED: n = 1 or n > 4096, or more than 2^31 - 1
 * workgroups.  The detail is read with fwa_last_error_string(NULL). */
int32_t fwc_describe(uint32_t n, uint64_t batch, int32_t *threads, int32_t *lds_bytes, int32_t *rows_per_block,
                     uint64_t *blocks);

/* kind: FWA_INVERSE_SCALED or FWA_INVERSE_UNSCALED; flags: 0 or FWC_CONJ_FILTER.
 * FWA_ERR_INVALID_ARG: a NULL handle, FWA_FORWARD, FWA_NORMALIZE or an unknown kind, unknown flag bits, n 0 or not a power
 * of two, a buffer of another context or of a destroyed one, a buffer size that is not a whole number of rows (or no row
 * at all, for the filter), src and dst sizes that differ, src and dst that overlap without being the same handle, a
 * filter that overlaps dst.  FWA_ERR_UNSUPPORTED: as fwc_describe. */
int32_t fwc_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t flags, uint32_t n, fwa_buf *src, fwa_buf *filter, fwa_buf *dst,
                        fwc_plan **out);

/* One launch, asynchronous, stream-ordered on `stream` (a stream of the plan's context; NULL = the null stream),
 * allocates nothing.  FWA_ERR_INVALID_ARG: a NULL plan, a stream of another context or of a destroyed one. */
int32_t fwc_plan_exec(fwc_plan *plan, fwa_stream *stream);

/* Keys: "fft_len", "batch", "filters" (F), "in_place" (1 when dst is src), "launches_per_exec" (always 1), "threads",
 * "lds_bytes", "rows_per_block", "blocks" (what fwc_describe answers). */
int32_t fwc_plan_get_i64(const fwc_plan *plan, const char *key, int64_t *value);

int32_t fwc_plan_destroy(fwc_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FFT_WGPU_AMD_CONV_H */
