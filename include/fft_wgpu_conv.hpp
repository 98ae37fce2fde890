// fft_wgpu_conv.hpp -- header-only C++ mirror of fft_wgpu_amd_conv.h: Convolve / OnlyConvolve, ifft(fft(x) * H) of batched
// rows in one launch, on the Device / Buffer / CommandEncoder of fft_wgpu.hpp.
//
//   fft_wgpu::Buffer x(dev, 8ull * count * 1024);                      // `count` rows of 1024 {re, im}
//   fft_wgpu::Buffer bank(dev, 8ull * 64 * 1024);                      // 64 filter spectra: row b uses spectrum b % 64
//   fft_wgpu::conv::Convolve fir(dev, dev, x, bank, x, 1024);          // src, filter, dst, fft_len; dst = src: in place
//   fir.proc(enc);                                                     // the result is `x`; `bank` is not written
//
// Link with -lfft_wgpu_amd_conv -lfft_wgpu_amd.  Errors throw fft_wgpu::Error.
#pragma once
#include "fft_wgpu.hpp"
#include "fft_wgpu_amd_conv.h"

namespace fft_wgpu {
namespace conv {

struct Geometry {
    int32_t threads = 0, lds_bytes = 0, rows_per_block = 0;
    uint64_t blocks = 0;
};

// fwc_describe: what a plan of this length launches; pure host logic, no device needed
inline Geometry describe(uint32_t fft_len, uint64_t batch = 1)
{
    Geometry g;
    const int32_t st = fwc_describe(fft_len, batch, &g.threads, &g.lds_bytes, &g.rows_per_block, &g.blocks);
    if (st) throw Error(st, std::string("fwc_describe: ") + fwa_last_error_string(nullptr));
    return g;
}

namespace detail {
class Plan {
public:
    Plan(const Device &d, int32_t kind, Buffer &src, Buffer &filter, Buffer &dst, uint32_t fft_len, bool conj_filter)
        : fft_len(fft_len), d_(d), dst_(dst)
    {
        const int32_t got = fwc_abi_version();
        if (got != FWC_ABI_VERSION)
            throw Error(FWA_ERR_UNSUPPORTED, "libfft_wgpu_amd_conv.so reports ABI version " + std::to_string(got) +
                                                 ", this header was written for version " + std::to_string(FWC_ABI_VERSION));
        d.check(fwc_plan_create(d.raw(), kind, conj_filter ? FWC_CONJ_FILTER : 0u, fft_len, src.raw(), filter.raw(), dst.raw(), &h_),
                "fwc_plan_create");
    }
    ~Plan() { fwc_plan_destroy(h_); }
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    // the dst buffer the plan was created on holds the result (src itself for an in-place plan)
    Buffer &proc(CommandEncoder &enc)
    {
        d_.check(fwc_plan_exec(h_, enc.raw()), "fwc_plan_exec");
        return dst_;
    }
    // fwc_plan_get_i64 ("fft_len", "batch", "filters", "in_place", "launches_per_exec", "threads", "lds_bytes",
    // "rows_per_block", "blocks")
    int64_t get(const char *key) const
    {
        int64_t v = 0;
        d_.check(fwc_plan_get_i64(h_, key, &v), "fwc_plan_get_i64");
        return v;
    }
    const uint32_t fft_len;

private:
    const Device &d_;
    Buffer &dst_;
    fwc_plan *h_ = nullptr;
};
}  // namespace detail

struct Convolve : detail::Plan {  // numpy.fft.ifft(numpy.fft.fft(x) * H) of every row
    Convolve(const Device &device, const Queue &, Buffer &src, Buffer &filter, Buffer &dst, uint32_t fft_len, bool conj_filter = false)
        : Plan(device, FWA_INVERSE_SCALED, src, filter, dst, fft_len, conj_filter) {}
};
struct OnlyConvolve : detail::Plan {  // fft_len times that: no scaling
    OnlyConvolve(const Device &device, const Queue &, Buffer &src, Buffer &filter, Buffer &dst, uint32_t fft_len, bool conj_filter = false)
        : Plan(device, FWA_INVERSE_UNSCALED, src, filter, dst, fft_len, conj_filter) {}
};

}  // namespace conv
}  // namespace fft_wgpu
