// fft_wgpu_stft.hpp -- header-only C++ mirror of fft_wgpu_amd_stft.h: Spectrum / Power over overlapping, windowed frames of
// long REAL signals, out of place, on the Device / Buffer / CommandEncoder of fft_wgpu.hpp.
//
//   fft_wgpu::Buffer audio(dev, 4ull * signals * len);                   // `signals` signals of `len` f32
//   fft_wgpu::Buffer hann(dev, 4ull * 1024);                             // 1024 f32
//   uint64_t frames = signals * fft_wgpu::stft::describe(1024, 256, len, signals).frames_per_signal;
//   fft_wgpu::Buffer spectra(dev, 8ull * frames * 513);                  // one row of 513 {re, im} per frame
//   fft_wgpu::stft::Spectrum stft(dev, dev, audio, spectra, 1024, 256, len, &hann);   // src, dst, fft_len, hop, signal_len, window
//   stft.proc(enc);                                                      // the result is `spectra`; `audio` and `hann` are not written
//
// Link with -lfft_wgpu_amd_stft -lfft_wgpu_amd.  Errors throw fft_wgpu::Error.
#pragma once
#include "fft_wgpu.hpp"
#include "fft_wgpu_amd_stft.h"

namespace fft_wgpu {
namespace stft {

struct Geometry {
    uint64_t frames_per_signal = 0;
    int32_t threads = 0, lds_bytes = 0, frames_per_block = 0;
    uint64_t blocks = 0;
};

// fwt_describe: what a plan of this shape launches; pure host logic, no device needed
inline Geometry describe(uint32_t fft_len, uint32_t hop, uint64_t signal_len, uint64_t signals = 1)
{
    Geometry g;
    const int32_t st = fwt_describe(fft_len, hop, signal_len, signals, &g.frames_per_signal, &g.threads, &g.lds_bytes,
                                    &g.frames_per_block, &g.blocks);
    if (st) throw Error(st, std::string("fwt_describe: ") + fwa_last_error_string(nullptr));
    return g;
}

namespace detail {
class Plan {
public:
    Plan(const Device &d, int32_t output, Buffer &src, Buffer &dst, uint32_t fft_len, uint32_t hop, uint64_t signal_len, Buffer *window)
        : fft_len(fft_len), hop(hop), signal_len(signal_len), d_(d), dst_(dst)
    {
        const int32_t got = fwt_abi_version();
        if (got != FWT_ABI_VERSION)
            throw Error(FWA_ERR_UNSUPPORTED, "libfft_wgpu_amd_stft.so reports ABI version " + std::to_string(got) +
                                                 ", this header was written for version " + std::to_string(FWT_ABI_VERSION));
        d.check(fwt_plan_create(d.raw(), output, fft_len, hop, signal_len, src.raw(), window ? window->raw() : nullptr, dst.raw(), &h_),
                "fwt_plan_create");
    }
    ~Plan() { fwt_plan_destroy(h_); }
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    // out of place: the dst buffer the plan was created on holds the result
    Buffer &proc(CommandEncoder &enc)
    {
        d_.check(fwt_plan_exec(h_, enc.raw()), "fwt_plan_exec");
        return dst_;
    }
    // fwt_plan_get_i64 ("fft_len", "hop", "signal_len", "signals", "frames_per_signal", "frames", "output", "windowed",
    // "launches_per_exec", "threads", "lds_bytes", "frames_per_block", "blocks")
    int64_t get(const char *key) const
    {
        int64_t v = 0;
        d_.check(fwt_plan_get_i64(h_, key, &v), "fwt_plan_get_i64");
        return v;
    }
    const uint32_t fft_len, hop;
    const uint64_t signal_len;

private:
    const Device &d_;
    Buffer &dst_;
    fwt_plan *h_ = nullptr;
};
}  // namespace detail

// window: nullptr = rectangular, else a buffer of fft_len f32, read on every exec
struct Spectrum : detail::Plan {  // numpy.fft.rfft of every windowed frame
    Spectrum(const Device &device, const Queue &, Buffer &src, Buffer &dst, uint32_t fft_len, uint32_t hop, uint64_t signal_len,
             Buffer *window = nullptr)
        : Plan(device, FWT_SPECTRUM, src, dst, fft_len, hop, signal_len, window) {}
};
struct Power : detail::Plan {  // re^2 + im^2 of the same bins
    Power(const Device &device, const Queue &, Buffer &src, Buffer &dst, uint32_t fft_len, uint32_t hop, uint64_t signal_len,
          Buffer *window = nullptr)
        : Plan(device, FWT_POWER, src, dst, fft_len, hop, signal_len, window) {}
};

}  // namespace stft
}  // namespace fft_wgpu
