/*
 * fft_wgpu_amd_strided.h -- C ABI of the strided-batch plans: the columns of a row-major matrix, transformed in place.
 *
 * The plans of fft_wgpu_amd.h take their transforms back to back (transform b starts at element b*fft_len).  A strided
 * plan takes the other everyday layout: `batch` row-major matrices of fft_len rows x howmany columns back to back, element
 * (j, c) of a matrix at j*howmany + c, and every column c becomes its own DFT over j -- numpy.fft.fft(x, axis=0), the
 * stride = howmany / dist = 1 case of FFTW's advanced interface: the Doppler axis of a pulses x range-bins cube,
 * interleaved channels, the second half of a 2-D transform (run an fwa_plan over the rows, then an fws_plan over the
 * columns of the same buffer: no transpose in between).  One launch, one pass over memory.
 *
 * Built into fft_wgpu_amd/libfft_wgpu_amd_strided.so (make -C fft_wgpu_amd/strided), which links against
 * libfft_wgpu_amd.so: contexts, buffers, streams, status codes and fwa_last_error_string are those of fft_wgpu_amd.h.
 * Plain C99; nothing throws or aborts across this boundary.
 *
 * Supported: fft_len = every power of two from 2 to 4096, howmany = any positive integer, matrices of any size (offsets
 * are 64-bit; a matrix may exceed 4 GiB).  Elements are {f32 re, f32 im} as in fft_wgpu_amd.h.
 *
 * Result: ALWAYS in `buf`, in natural order -- row k of column c at k*howmany + c.  These plans have no reference
 * analogue, so the reference's odd/even rule for the result buffer (fwa_plan_exec) does not apply and there is no second
 * buffer.
 *
 * Lifetimes as in fft_wgpu_amd.h: a plan goes before its context, and the buffer outlives the plan.
 *
 * Launch geometry (fws_describe, and the same keys of fws_plan_get_i64): a workgroup owns tiles of `tile_cols` adjacent
 * columns by all fft_len rows of one matrix.  With tiles = ceil(howmany / tile_cols) per matrix,
 *     blocks = batch * ceil(tiles / tiles_per_workgroup),
 * where tiles_per_workgroup = 512 / fft_len for fft_len <= 32 (a thread holds a whole column; a workgroup moves 64 KiB)
 * and 1 above.  tile_cols is 16, except 8 at fft_len = 4096.
 */
#ifndef FFT_WGPU_AMD_STRIDED_H
#define FFT_WGPU_AMD_STRIDED_H

#include "fft_wgpu_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FWS_ABI_VERSION 1

typedef struct fws_plan fws_plan;

int32_t fws_abi_version(void);

/* Pure host logic, no device: the launch geometry a plan of this shape uses.  Any output pointer may be NULL.
 * FWA_ERR_INVALID_ARG: fft_len 0 or not a power of two, howmany = 0; FWA_ERR_UNSUPPORTED: fft_len = 1 or fft_len > 4096,
 * or more than 2^31 - 1 blocks.  The detail is read with fwa_last_error_string(NULL). */
int32_t fws_describe(uint32_t fft_len, uint64_t howmany, uint64_t batch,
                     int32_t *tile_cols, int32_t *threads, int32_t *lds_bytes, uint64_t *blocks);

/* kind: FWA_FORWARD, FWA_INVERSE_SCALED (times 2^-log2 fft_len, fused into the last stage) or FWA_INVERSE_UNSCALED.
 * buf holds `batch` matrices of fft_len rows x howmany columns back to back; batch = fwa_buf_size(buf) / (8 * fft_len *
 * howmany).  FWA_ERR_INVALID_ARG: a NULL handle, fft_len 0 or not a power of two, howmany = 0, a buffer size that is not
 * a whole number of matrices, FWA_NORMALIZE or an unknown kind, a buffer of another context or of a destroyed one.
 * FWA_ERR_UNSUPPORTED: fft_len = 1 or fft_len > 4096. */
int32_t fws_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t fft_len, uint64_t howmany, fwa_buf *buf, fws_plan **out);

/* In place, asynchronous, stream-ordered on `stream` (a stream of the plan's context; NULL = the null stream), allocates
 * nothing.  FWA_ERR_INVALID_ARG: a NULL plan, a stream of another context or of a destroyed one. */
int32_t fws_plan_exec(fws_plan *plan, fwa_stream *stream);

/* Keys: "fft_len", "howmany", "batch"; "tile_cols", "threads", "lds_bytes", "blocks" (what fws_describe answers);
 * "launches_per_exec" (1 for every supported shape). */
int32_t fws_plan_get_i64(const fws_plan *plan, const char *key, int64_t *value);

int32_t fws_plan_destroy(fws_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FFT_WGPU_AMD_STRIDED_H */
