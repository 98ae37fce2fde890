// fft_wgpu_strided.hpp -- header-only C++ mirror of fft_wgpu_amd_strided.h: Forward / Inverse / Onlyinverse over the
// COLUMNS of row-major matrices, on the Device / Buffer / CommandEncoder of fft_wgpu.hpp.
//
//   fft_wgpu::Buffer cube(dev, 8ull * pulses * bins);                 // pulses rows x bins columns, row-major
//   fft_wgpu::strided::Forward doppler(dev, dev, cube, pulses, bins);  // fft_len = pulses, howmany = bins
//   doppler.proc(enc);                                                 // in place: the result is `cube`
//
// Link with -lfft_wgpu_amd_strided -lfft_wgpu_amd.  Errors throw fft_wgpu::Error.
#pragma once
#include "fft_wgpu.hpp"
#include "fft_wgpu_amd_strided.h"

namespace fft_wgpu {
namespace strided {

struct Geometry {
    int32_t tile_cols = 0, threads = 0, lds_bytes = 0;
    uint64_t blocks = 0;
};

// fws_describe: the launch geometry a plan of this shape uses; pure host logic, no device needed
inline Geometry describe(uint32_t fft_len, uint64_t howmany, uint64_t batch = 1)
{
    Geometry g;
    const int32_t st = fws_describe(fft_len, howmany, batch, &g.tile_cols, &g.threads, &g.lds_bytes, &g.blocks);
    if (st) throw Error(st, std::string("fws_describe: ") + fwa_last_error_string(nullptr));
    return g;
}

namespace detail {
class Plan {
public:
    Plan(const Device &d, int32_t kind, Buffer &src, uint32_t fft_len, uint64_t howmany)
        : fft_len(fft_len), howmany(howmany), d_(d), src_(src)
    {
        const int32_t got = fws_abi_version();
        if (got != FWS_ABI_VERSION)
            throw Error(FWA_ERR_UNSUPPORTED, "libfft_wgpu_amd_strided.so reports ABI version " + std::to_string(got) +
                                                 ", this header was written for version " + std::to_string(FWS_ABI_VERSION));
        d.check(fws_plan_create(d.raw(), kind, fft_len, howmany, src.raw(), &h_), "fws_plan_create");
    }
    ~Plan() { fws_plan_destroy(h_); }
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    // in place: the buffer the plan was created on holds the result
    Buffer &proc(CommandEncoder &enc)
    {
        d_.check(fws_plan_exec(h_, enc.raw()), "fws_plan_exec");
        return src_;
    }
    // fws_plan_get_i64 ("tile_cols", "threads", "lds_bytes", "blocks", "batch", "launches_per_exec", ...)
    int64_t get(const char *key) const
    {
        int64_t v = 0;
        d_.check(fws_plan_get_i64(h_, key, &v), "fws_plan_get_i64");
        return v;
    }
    const uint32_t fft_len;
    const uint64_t howmany;

private:
    const Device &d_;
    Buffer &src_;
    fws_plan *h_ = nullptr;
};
}  // namespace detail

struct Forward : detail::Plan {  // unnormalised forward DFT of every column
    Forward(const Device &device, const Queue &, Buffer &src, uint32_t fft_len, uint64_t howmany)
        : Plan(device, FWA_FORWARD, src, fft_len, howmany) {}
};
struct Inverse : detail::Plan {  // inverse DFT of every column, 1 / fft_len fused
    Inverse(const Device &device, const Queue &, Buffer &src, uint32_t fft_len, uint64_t howmany)
        : Plan(device, FWA_INVERSE_SCALED, src, fft_len, howmany) {}
};
struct Onlyinverse : detail::Plan {  // inverse DFT of every column, unscaled
    Onlyinverse(const Device &device, const Queue &, Buffer &src, uint32_t fft_len, uint64_t howmany)
        : Plan(device, FWA_INVERSE_UNSCALED, src, fft_len, howmany) {}
};

}  // namespace strided
}  // namespace fft_wgpu
