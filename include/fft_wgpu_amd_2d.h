/*
 * fft_wgpu_amd_2d.h -- C ABI of the 2-D plans: batched row-major images, transformed in place.
 *
 * `buf` holds `batch` row-major images of rows x cols back to back: element (j, c) of image b at (b*rows + j)*cols + c,
 * batch = fwa_buf_size(buf) / (8 * rows * cols).  A plan computes numpy.fft.fft2 / ifft2 over the last two axes of that
 * (batch, rows, cols) array.  Elements are {f32 re, f32 im} as in fft_wgpu_amd.h.
 *
 * Result: ALWAYS in `buf`, in natural order, for every width: there is no second buffer, and the odd/even rule of
 * fwa_plan_exec does not apply.
 *
 * Built into fft_wgpu_amd/libfft_wgpu_amd_2d.so (make -C fft_wgpu_amd/fft2d), which links against
 * libfft_wgpu_amd_strided.so and libfft_wgpu_amd.so: contexts, buffers, streams, status codes and fwa_last_error_string are
 * those of fft_wgpu_amd.h, and the column pass is a strided-batch plan (fft_wgpu_amd_strided.h) the 2-D plan owns.
 * Plain C99; nothing throws or aborts across this boundary.
 *
 * Supported: rows and cols = every power of two from 2 to 4096, in any combination; buffers of any size (a buffer may
 * exceed 4 GiB).  rows = 1 or cols = 1 is a 1-D transform: FWA_ERR_UNSUPPORTED, use fwa_plan / fws_plan.
 *
 * What runs (fw2_describe, and the same keys of fw2_plan_get_i64):
 *     rows <= 32 and cols <= 32   1 launch, 16 bytes of traffic per sample: rows, then columns, inside the 64-KiB chunk
 *                                 of 8192 samples one 256-thread workgroup moves; row_blocks = ceil(batch*rows*cols / 8192)
 *     cols <= 32, rows >= 64      2 launches: the same kernel, rows only; then the strided-batch plan over the columns
 *     cols >= 64                  2 launches: a row kernel with RT adjacent rows of the buffer per workgroup (RT = 16, 8 at
 *                                 cols = 4096; a tile may span two images), row_blocks = ceil(batch*rows / RT); then the
 *                                 strided-batch plan over the columns
 *
 * Lifetimes as in fft_wgpu_amd.h: a plan goes before its context, and the buffer outlives the plan.
 */
#ifndef FFT_WGPU_AMD_2D_H
#define FFT_WGPU_AMD_2D_H

#include "fft_wgpu_amd_strided.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FW2_ABI_VERSION 1

typedef struct fw2_plan fw2_plan;

int32_t fw2_abi_version(void);

/* Pure host logic, no device: what a plan of this shape launches.  launches: 1 or 2; row_threads, row_lds_bytes,
 * row_blocks: workgroup size, dynamic LDS and grid of the row launch.  Any output pointer may be NULL.
 * FWA_ERR_INVALID_ARG: rows or cols 0 or not a power of two; FWA_ERR_UNSUPPORTED: rows or cols = 1 (the detail names the
 * 1-D plans) or > 4096, or more than 2^31 - 1 workgroups in a launch.  The detail is read with
 * fwa_last_error_string(NULL). */
int32_t fw2_describe(uint32_t rows, uint32_t cols, uint64_t batch,
                     int32_t *launches, int32_t *row_threads, int32_t *row_lds_bytes, uint64_t *row_blocks);

/* kind: FWA_FORWARD, FWA_INVERSE_SCALED (times 2^-(log2 rows + log2 cols): the row pass multiplies by 1 / cols, the
 * column pass by 1 / rows, both exact) or FWA_INVERSE_UNSCALED.  FWA_ERR_INVALID_ARG: a NULL handle, rows or cols 0 or
 * not a power of two, a buffer size that is not a whole number of images, FWA_NORMALIZE or an unknown kind, a buffer of
 * another context or of a destroyed one, a buffer base that is not 16-byte aligned (every row then starts 16-byte
 * aligned).  FWA_ERR_UNSUPPORTED: as fw2_describe. */
int32_t fw2_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t rows, uint32_t cols, fwa_buf *buf, fw2_plan **out);

/* In place, asynchronous, stream-ordered on `stream` (a stream of the plan's context; NULL = the null stream), allocates
 * nothing.  FWA_ERR_INVALID_ARG: a NULL plan, a stream of another context or of a destroyed one. */
int32_t fw2_plan_exec(fw2_plan *plan, fwa_stream *stream);

/* Keys: "rows", "cols", "batch"; "launches_per_exec" (1 or 2); "row_threads", "row_lds_bytes", "row_blocks" (what
 * fw2_describe answers); "col_blocks" (the grid of the column launch; 0 on the one-launch path). */
int32_t fw2_plan_get_i64(const fw2_plan *plan, const char *key, int64_t *value);

int32_t fw2_plan_destroy(fw2_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FFT_WGPU_AMD_2D_H */
