/*
 * fft_wgpu_amd_stft.h -- C ABI of the framed real-input plans: the rfft of overlapping, windowed frames of long real signals
 * (the frames of a spectrogram, scipy.signal.stft, torch.stft(..., center=False, onesided=True)), out of place, in one
 * launch.  Forward only.
 *
 * With n a power of two, M = n / 2, hop >= 1 (it may be odd and it may exceed n) and L >= n:
 *   `src` holds `signals` signals of L f32 back to back.  A signal has F = 1 + (L - n) / hop frames (integer division; a tail
 *   that fills no frame is never read); frame f of signal s is the n floats from float s L + f hop on, and it is frame
 *   g = s F + f of the plan.  `dst` receives frame g as row g, signal-major, no padding:
 *     numpy.fft.rfft(w * numpy.lib.stride_tricks.sliding_window_view(x, n, axis=-1)[:, ::hop], axis=-1)
 *   FWT_SPECTRUM   rows of M + 1 samples {f32 re, f32 im}, bins 0 .. n/2; Im X[0] and Im X[M] are stored as 0.0f, as
 *                  fft_wgpu_amd_real.h's forward plans store them
 *   FWT_POWER      rows of M + 1 f32, re^2 + im^2 of the same bins (rows start only 4-byte aligned)
 *   `window`       n f32 (exactly 4 n bytes), multiplied onto every frame in f32 before the transform; it is read on every
 *                  exec, stream-ordered, so it may be rewritten between execs.  NULL: rectangular, no product is formed.
 *
 * signals = fwa_buf_size(src) / (4 L), which must divide evenly; fwa_buf_size(dst) must be signals F rows of the chosen
 * output.  Plans are always out of place: `src` and `window` are never written, and a `src` or a `window` whose byte range
 * overlaps `dst`'s is refused.  Any buffer may exceed 4 GiB.
 *
 * Built into fft_wgpu_amd/libfft_wgpu_amd_stft.so (make -C fft_wgpu_amd/stft), which links against libfft_wgpu_amd.so:
 * contexts, buffers, streams, status codes and fwa_last_error_string are those of fft_wgpu_amd.h.  Plain C99; nothing
 * throws or aborts across this boundary.
 *
 * Supported: n = every power of two from 2 to 4096.  What runs (fwt_describe, and the same keys of fwt_plan_get_i64) is the
 * geometry of the real-input plans of the same n, a frame taking the place of a row:
 *     n = 2 .. 64       one frame per thread, 256 frames per 256-thread workgroup: blocks = ceil(frames / 256)
 *     n = 128 .. 4096   16 adjacent frames per workgroup on the M-point network, blocks = ceil(frames / 16)
 *
 * Lifetimes as in fft_wgpu_amd.h: a plan goes before its context, and the buffers outlive the plan.
 */
#ifndef FFT_WGPU_AMD_STFT_H
#define FFT_WGPU_AMD_STFT_H

#include "fft_wgpu_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FWT_ABI_VERSION 1

/* what a plan stores per bin */
#define FWT_SPECTRUM 0
#define FWT_POWER 1

typedef struct fwt_plan fwt_plan;

int32_t fwt_abi_version(void);

/* Pure host logic, no device: what a plan of length n launches over `signals` signals of signal_len f32 at this hop.
 * frames_per_signal: F; threads, lds_bytes: workgroup size and dynamic LDS; frames_per_block: frames one workgroup owns;
 * blocks = ceil(signals F / frames_per_block).  Any output pointer may be NULL.  FWA_ERR_INVALID_ARG: n 0 or not a power of
 * two, hop = 0, signal_len < n, sizes that overflow 64 bits; FWA_ERR_UNSUPPORTED: n = 1 or n > 4096, or more than 2^31 - 1
 * workgroups.  The detail is read with fwa_last_error_string(NULL). */
int32_t fwt_describe(uint32_t n, uint32_t hop, uint64_t signal_len, uint64_t signals, uint64_t *frames_per_signal, int32_t *threads,
                     int32_t *lds_bytes, int32_t *frames_per_block, uint64_t *blocks);

/* output: FWT_SPECTRUM or FWT_POWER.  window: NULL or a buffer of exactly 4 n bytes.
 * FWA_ERR_INVALID_ARG: a NULL ctx / src / dst / out, n 0 or not a power of two, an unknown output, hop = 0, signal_len < n,
 * a buffer of another context or of a destroyed one, a src size that is not a whole number of signals, a dst size other than
 * signals F rows of the chosen output, a window of another size, a src or a window whose byte range overlaps dst's.
 * FWA_ERR_UNSUPPORTED: as fwt_describe. */
int32_t fwt_plan_create(fwa_ctx *ctx, int32_t output, uint32_t n, uint32_t hop, uint64_t signal_len, fwa_buf *src, fwa_buf *window,
                        fwa_buf *dst, fwt_plan **out);

/* One launch, asynchronous, stream-ordered on `stream` (a stream of the plan's context; NULL = the null stream),
 * allocates nothing.  FWA_ERR_INVALID_ARG: a NULL plan, a stream of another context or of a destroyed one. */
int32_t fwt_plan_exec(fwt_plan *plan, fwa_stream *stream);

/* Keys: "fft_len", "hop", "signal_len", "signals", "frames_per_signal", "frames" (= signals * frames_per_signal), "output",
 * "windowed" (0 or 1), "launches_per_exec" (always 1), "threads", "lds_bytes", "frames_per_block", "blocks" (what
 * fwt_describe answers). */
int32_t fwt_plan_get_i64(const fwt_plan *plan, const char *key, int64_t *value);

int32_t fwt_plan_destroy(fwt_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* FFT_WGPU_AMD_STFT_H */
