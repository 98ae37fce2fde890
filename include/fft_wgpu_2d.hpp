// fft_wgpu_2d.hpp -- header-only C++ mirror of fft_wgpu_amd_2d.h: Forward / Inverse / Onlyinverse over batched row-major
// IMAGES, in place, on the Device / Buffer / CommandEncoder of fft_wgpu.hpp.
//
//   fft_wgpu::Buffer tiles(dev, 8ull * count * 32 * 32);             // `count` images of 32 rows x 32 columns
//   fft_wgpu::fft2d::Forward fft2(dev, dev, tiles, 32, 32);           // rows, cols
//   fft2.proc(enc);                                                    // in place: the result is `tiles`
//
// Link with -lfft_wgpu_amd_2d -lfft_wgpu_amd_strided -lfft_wgpu_amd.  Errors throw fft_wgpu::Error.
#pragma once
#include "fft_wgpu.hpp"
#include "fft_wgpu_amd_2d.h"

namespace fft_wgpu {
namespace fft2d {

struct Geometry {
    int32_t launches = 0, row_threads = 0, row_lds_bytes = 0;
    uint64_t row_blocks = 0;
};

// fw2_describe: what a plan of this shape launches; pure host logic, no device needed
inline Geometry describe(uint32_t rows, uint32_t cols, uint64_t batch = 1)
{
    Geometry g;
    const int32_t st = fw2_describe(rows, cols, batch, &g.launches, &g.row_threads, &g.row_lds_bytes, &g.row_blocks);
    if (st) throw Error(st, std::string("fw2_describe: ") + fwa_last_error_string(nullptr));
    return g;
}

namespace detail {
class Plan {
public:
    Plan(const Device &d, int32_t kind, Buffer &src, uint32_t rows, uint32_t cols) : rows(rows), cols(cols), d_(d), src_(src)
    {
        const int32_t got = fw2_abi_version();
        if (got != FW2_ABI_VERSION)
            throw Error(FWA_ERR_UNSUPPORTED, "libfft_wgpu_amd_2d.so reports ABI version " + std::to_string(got) +
                                                 ", this header was written for version " + std::to_string(FW2_ABI_VERSION));
        d.check(fw2_plan_create(d.raw(), kind, rows, cols, src.raw(), &h_), "fw2_plan_create");
    }
    ~Plan() { fw2_plan_destroy(h_); }
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    // in place: the buffer the plan was created on holds the result
    Buffer &proc(CommandEncoder &enc)
    {
        d_.check(fw2_plan_exec(h_, enc.raw()), "fw2_plan_exec");
        return src_;
    }
    // fw2_plan_get_i64 ("launches_per_exec", "row_threads", "row_lds_bytes", "row_blocks", "col_blocks", "batch", ...)
    int64_t get(const char *key) const
    {
        int64_t v = 0;
        d_.check(fw2_plan_get_i64(h_, key, &v), "fw2_plan_get_i64");
        return v;
    }
    const uint32_t rows, cols;

private:
    const Device &d_;
    Buffer &src_;
    fw2_plan *h_ = nullptr;
};
}  // namespace detail

struct Forward : detail::Plan {  // unnormalised forward 2-D DFT of every image
    Forward(const Device &device, const Queue &, Buffer &src, uint32_t rows, uint32_t cols)
        : Plan(device, FWA_FORWARD, src, rows, cols) {}
};
struct Inverse : detail::Plan {  // inverse 2-D DFT of every image, times 1 / (rows * cols)
    Inverse(const Device &device, const Queue &, Buffer &src, uint32_t rows, uint32_t cols)
        : Plan(device, FWA_INVERSE_SCALED, src, rows, cols) {}
};
struct Onlyinverse : detail::Plan {  // inverse 2-D DFT of every image, unscaled
    Onlyinverse(const Device &device, const Queue &, Buffer &src, uint32_t rows, uint32_t cols)
        : Plan(device, FWA_INVERSE_UNSCALED, src, rows, cols) {}
};

}  // namespace fft2d
}  // namespace fft_wgpu
