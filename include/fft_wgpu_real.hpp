// fft_wgpu_real.hpp -- header-only C++ mirror of fft_wgpu_amd_real.h: Forward / Inverse / Onlyinverse over batched REAL
// rows, out of place, on the Device / Buffer / CommandEncoder of fft_wgpu.hpp.
//
//   fft_wgpu::Buffer frames(dev, 4ull * count * 1024);                 // `count` rows of 1024 f32
//   fft_wgpu::Buffer spectra(dev, 8ull * count * 513);                 // `count` rows of 513 {re, im}: bins 0 .. 512
//   fft_wgpu::real::Forward rfft(dev, dev, frames, spectra, 1024);     // src, dst, fft_len
//   rfft.proc(enc);                                                    // the result is `spectra`; `frames` is not written
//
// Link with -lfft_wgpu_amd_real -lfft_wgpu_amd.  Errors throw fft_wgpu::Error.
#pragma once
#include "fft_wgpu.hpp"
#include "fft_wgpu_amd_real.h"

namespace fft_wgpu {
namespace real {

struct Geometry {
    int32_t threads = 0, lds_bytes = 0, rows_per_block = 0;
    uint64_t blocks = 0;
};

// fwr_describe: what a plan of this length launches; pure host logic, no device needed
inline Geometry describe(uint32_t fft_len, uint64_t batch = 1)
{
    Geometry g;
    const int32_t st = fwr_describe(fft_len, batch, &g.threads, &g.lds_bytes, &g.rows_per_block, &g.blocks);
    if (st) throw Error(st, std::string("fwr_describe: ") + fwa_last_error_string(nullptr));
    return g;
}

namespace detail {
class Plan {
public:
    Plan(const Device &d, int32_t kind, Buffer &src, Buffer &dst, uint32_t fft_len) : fft_len(fft_len), d_(d), dst_(dst)
    {
        const int32_t got = fwr_abi_version();
        if (got != FWR_ABI_VERSION)
            throw Error(FWA_ERR_UNSUPPORTED, "libfft_wgpu_amd_real.so reports ABI version " + std::to_string(got) +
                                                 ", this header was written for version " + std::to_string(FWR_ABI_VERSION));
        d.check(fwr_plan_create(d.raw(), kind, fft_len, src.raw(), dst.raw(), &h_), "fwr_plan_create");
    }
    ~Plan() { fwr_plan_destroy(h_); }
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    // out of place: the dst buffer the plan was created on holds the result
    Buffer &proc(CommandEncoder &enc)
    {
        d_.check(fwr_plan_exec(h_, enc.raw()), "fwr_plan_exec");
        return dst_;
    }
    // fwr_plan_get_i64 ("fft_len", "batch", "launches_per_exec", "threads", "lds_bytes", "rows_per_block", "blocks")
    int64_t get(const char *key) const
    {
        int64_t v = 0;
        d_.check(fwr_plan_get_i64(h_, key, &v), "fwr_plan_get_i64");
        return v;
    }
    const uint32_t fft_len;

private:
    const Device &d_;
    Buffer &dst_;
    fwr_plan *h_ = nullptr;
};
}  // namespace detail

struct Forward : detail::Plan {  // numpy.fft.rfft of every row
    Forward(const Device &device, const Queue &, Buffer &src, Buffer &dst, uint32_t fft_len)
        : Plan(device, FWA_FORWARD, src, dst, fft_len) {}
};
struct Inverse : detail::Plan {  // numpy.fft.irfft of every row
    Inverse(const Device &device, const Queue &, Buffer &src, Buffer &dst, uint32_t fft_len)
        : Plan(device, FWA_INVERSE_SCALED, src, dst, fft_len) {}
};
struct Onlyinverse : detail::Plan {  // fft_len * numpy.fft.irfft of every row
    Onlyinverse(const Device &device, const Queue &, Buffer &src, Buffer &dst, uint32_t fft_len)
        : Plan(device, FWA_INVERSE_UNSCALED, src, dst, fft_len) {}
};

}  // namespace real
}  // namespace fft_wgpu
