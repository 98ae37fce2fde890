// internal.h -- handles, shared helpers and the cross-file interface of the library's host side (not installed).
//
// The host side of the C ABI (include/fft_wgpu_amd.h) is split by concern:
//   ctx_streams.cpp  contexts, error strings, device enumeration, the slab rule, streams (+ the overlap check), events
//   buffers.cpp      device / pinned memory, uploads, downloads, copies (peer copies across contexts), synthetic data
//   tables.cpp       twiddle tables (reference twiddle rule src/processor.rs:43-49), the ring pool, build_pipeline /
//                    release_pipeline: the only code that allocates or frees what a Pipeline (below) holds
//   handles.h        which stream / buffer / event handles belong to which context, under one process-wide lock: no HIP
//   schedule.h       path choice, kernel limits and the kernel of every pass of a tiled plan: pure integer logic, no HIP
//   plan.cpp         plan create / destroy / exec (the four plan objects of src/processor.rs)
//   tuning.cpp       fwa_plan_get_i64 / fwa_plan_set_i64; every key that rebuilds the pipeline goes through retune()
//   comm.cpp         fwa_comm_*: slab movement over RCCL
//   kernels.h        the launch wrappers of kernels_*.hip: prototypes and argument structs, no device code
// Nothing above includes a device header (cplx.h, device_common.h, tile_*.h, rows32.h, small32_*.h): the host files are
// compiled once, as plain C++ against the HIP runtime API, and the same objects go into the product and the laboratory
// library.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/fft_wgpu_amd.h"
#include "handles.h"
#include "kernels.h"

using fwa::v2f;

// The laboratory library (libfft_wgpu_amd_lab.so, `make lab`): the same ABI plus the kernel families that measured slower
// than the shipped ones -- path 5 (persistent 2^20 ring), small_reg = 2 / 3 (direct 16-point kernels, wavefront-shuffle
// exchange) -- and two test knobs (ring_rotate, inject_launch_failure).  The product library rejects those settings.
// The two differ at link time only: the laboratory library links kernels_lab_*.hip (the laboratory launchers of kernels.h)
// and lab_present.cpp (kLab = true), the product lab_absent.cpp (kLab = false and stubs of those launchers).  Plain
// symbols, no table of function pointers: the host calls them by name like every other launcher, and fwa_plan_set_i64
// refuses, when !kLab, every key that leads to one.
using fwa::kLab;

namespace fwa_int {

// Device tables of one transform length, shared by every plan of that length on a context (plan cache):
// tables hold forward twiddles only (the inverse conjugates on use), so all plan kinds share them.
struct Tables {
    v2f *tw_half = nullptr;   // n/2 entries, processor.rs:43-49 (small / literal paths)
    v2f *tw_inner = nullptr;  // 2^20 path: [k1][n'] = W_1024^{n' k1}
    v2f *tw_outer = nullptr;  // 2^20 path: per 16-column tile A[32][16], B[32][16]
    v2f *tw_l[3] = {nullptr, nullptr, nullptr};  // tiled path: per-factor W_L tables
    v2f *tw_lo1 = nullptr, *tw_hi1 = nullptr;    // four-step tables of pass A (domain n)
    v2f *tw_lo_b = nullptr, *tw_hi_b = nullptr;  // four-step tables of pass B (domain N2*N3)
    ~Tables()
    {
        for (v2f *t : {tw_half, tw_inner, tw_outer, tw_l[0], tw_l[1], tw_l[2], tw_lo1, tw_hi1, tw_lo_b,
                       tw_hi_b})
            if (t) (void)hipFree(t);
    }
};

// What a pipelined plan (two-pass 2^20, tiled; laboratory: the persistent ring) runs on, and its geometry.  A plan has one;
// build_pipeline makes a new one and swaps it in, release_pipeline is the only code that frees any part of it.
struct Pipeline {
    v2f *ring = nullptr;               // scratch: group * n_streams [* ring_rotate] transforms
    uint64_t ring_bytes = 0;
    uint32_t *ctl = nullptr;           // PATH_RING_1M: ticket, error word, per-transform hand-off counters
    uint64_t ctl_bytes = 0;
    std::vector<hipStream_t> streams;  // chains the groups alternate over: borrowed from ctx->chains, empty for one chain
    std::vector<hipEvent_t> done;      // join event of every chain
    hipEvent_t fork = nullptr;
    int64_t group = 16;                // transforms per launch
    int64_t n_streams = 2;             // chains
};

}  // namespace fwa_int

struct fwa_ctx {
    int device = -1;
    hipDeviceProp_t prop{};
    mutable std::string err;
    uint32_t kernel_families = 0;  // kernel families whose dynamic-LDS limits are raised (plan.cpp: setup_path)
    // plan cache: (fft_len, path, factor signature) -> tables; ring allocations of destroyed plans by size
    std::map<std::tuple<uint32_t, int64_t, uint32_t>, std::shared_ptr<fwa_int::Tables>> tables;
    std::vector<std::pair<uint64_t, void *>> free_rings;  // rings of destroyed plans, oldest first
    uint64_t free_ring_bytes = 0;
    int64_t n_table_builds = 0, n_table_hits = 0, n_ring_allocs = 0, n_ring_reuses = 0, last_plan_create_us = 0;
    // Internal chain streams of the pipelined paths: created once per context, shared by every plan, and checked at
    // creation to run kernels side by side (chain_streams() below).
    std::vector<hipStream_t> chains;
    int64_t n_chain_checks = 0, n_chain_rejects = 0, chain_pair_us = 0, chain_single_us = 0;
    // fwa_ctx_set_i64("chain_check", 0): new streams are taken as the runtime hands them out
    int64_t chain_check = 1;
    std::vector<int> peers_enabled;         // device ordinals this context's device has peer access to (enabled once)
    // Every alive fwa_stream / fwa_buf / fwa_event handle of this context (created, allocated or wrapped), oldest first.
    // handles.h owns it and its lock; fwa_ctx_destroy detaches them all, so that a handle which outlives its context
    // (garbage-collected hosts free in any order, from any thread) answers FWA_ERR_INVALID_ARG and stays destroyable.
    fwa_int::HandleList handles;
};
// Handle::ctx is nullptr once the context has been destroyed: every entry point then refuses the handle, which can still
// be destroyed (LIVE_HANDLE below).
struct fwa_stream : fwa_int::Handle {
    hipStream_t s = nullptr;
    bool owned = false;
    int device = -1;
};
struct fwa_buf : fwa_int::Handle {
    void *p = nullptr;
    uint64_t bytes = 0;
    bool owned = false;
    int device = -1;          // for fwa_buf_free after the context is gone
};
struct fwa_event : fwa_int::Handle {
    hipEvent_t e = nullptr;
};

struct fwa_plan {
    fwa_ctx *ctx = nullptr;
    int32_t kind = 0;
    uint32_t n = 0;
    uint32_t lg = 0;
    uint64_t batch = 0;
    fwa_buf *src = nullptr;        // buffer_a (processor.rs:12,237,575) / buffer1 for Normalize
    fwa_buf *second = nullptr;     // buffer_b: plan-owned (Forward/Inverse) or caller's src2
    fwa_buf own_second;            // storage when plan-owned
    bool second_owned = false;
    int64_t path = PATH_R2_GLOBAL;
    bool frozen = false;           // first exec done -> tunables locked
    std::shared_ptr<fwa_int::Tables> tb;    // shared through ctx->tables
    v2f *tw_half_private = nullptr;  // forced literal path on a size whose cached tables have no n/2 table
    uint32_t lf[3] = {0, 0, 0};    // tiled path: log2 of the factors (lf[2] = 0 for two factors)
    fwa_int::Pipeline pipe;        // two-pass 2^20 and tiled paths: groups of transforms alternate over internal streams
    // XCD-aware block -> tile mapping (xcd_map bits): -1 = per-path, per-size default (swizzle_default, plan.cpp)
    int64_t xcd_swizzle = -1;
    fwa_int::TiledFlags flags;     // tiled plans: the keys "colsw", "rows32", "p1_gen", "tile_ring" (schedule.h)
    // laboratory: the ring is this many times larger and the groups rotate through it (same launches, larger cache
    // footprint: prices what the Infinity Cache gives the ring)
    int64_t ring_rotate = 1;
    // n <= 32768: 1 = k_chunk / k_small32; laboratory: 3 = direct 16-point kernels (16 .. 4096), 2 = + wave shuffles
    int64_t small_reg = 1;
    // the caller's stream of the last exec that used the ring: fwa_plan_destroy waits for the work enqueued there (an
    // event per exec would cost 4-5 us on the 1-3-launch latency shapes)
    hipStream_t last_stream = nullptr;
    bool ran_on_stream = false;
    // persistent 2^20 pipeline (PATH_RING_1M)
    int64_t depth = 8;             // pass-2 tiles of transform t run beside pass-1 tiles of transform t + depth
    int64_t ring_slots = 12;       // transforms of intermediate kept (>= depth + 1)
    int64_t wgs = 512;             // persistent workgroups (2 per CU)
    // laboratory: the launch of this group fails once (error path of run_groups under test)
    int64_t inject_fail_group = -1;
};

namespace fwa_int {

// ---- errors (ctx_streams.cpp): record the message on the context (or thread-locally without one), return the status
int32_t fail(const fwa_ctx *ctx, int32_t status, const std::string &msg);
int32_t fail_hip(const fwa_ctx *ctx, hipError_t e, const char *what, int32_t status = FWA_ERR_HIP);
const char *thread_error_string();

#define HIP_TRY(ctx, call)                                                \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return fwa_int::fail_hip((ctx), e_, #call); \
    } while (0)

// Every entry point that touches the device makes the context's device current first: with one context per
// device in one process work must not land on whichever device was used last.
#define USE_DEVICE(ctx)                                                                                   \
    do {                                                                                                  \
        int cur_ = -1;                                                                                    \
        if (hipGetDevice(&cur_) != hipSuccess || cur_ != (ctx)->device) HIP_TRY((ctx), hipSetDevice((ctx)->device)); \
    } while (0)

inline bool is_pow2(uint32_t n) { return n && !(n & (n - 1)); }
inline hipStream_t raw(fwa_stream *s) { return s ? s->s : nullptr; }

// A buffer / event handle whose context has been destroyed may still be freed, never used (include/fft_wgpu_amd.h,
// "Lifetimes"): every entry point that takes one starts with this check.  A plain read outside the registry lock: only
// FREEING a handle is safe while its context is being destroyed, using one concurrently stays the caller's error.
#define LIVE_HANDLE(h, what)                                                                              \
    do {                                                                                                  \
        if (!(h)->ctx)                                                                                    \
            return fwa_int::fail(nullptr, FWA_ERR_INVALID_ARG, what " belongs to a context that has been destroyed"); \
    } while (0)

// ---- ctx_streams.cpp ----
int32_t overlapping_stream(fwa_ctx *ctx, const std::vector<hipStream_t> &peers, hipStream_t *out);
int32_t chain_streams(fwa_ctx *ctx, size_t n);  // the context's chain streams, created (and checked) on demand

// ---- tables.cpp ----
int32_t upload_half_table(fwa_ctx *ctx, uint32_t n, v2f **d);
int32_t build_tables(fwa_ctx *ctx, uint32_t n, int64_t path, const uint32_t lf[3], Tables *t);
void release_pipeline(fwa_ctx *ctx, Pipeline &pl, bool pool_ring);
int32_t build_pipeline(fwa_plan *p, int64_t group, int64_t n_streams);

// ---- plan.cpp ----
int32_t setup_path(fwa_plan *p);
uint32_t swizzle_default(const fwa_plan *p);  // the block -> tile map of a pipelined plan while "xcd_swizzle" is unset

}  // namespace fwa_int
