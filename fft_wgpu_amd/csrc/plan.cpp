// plan.cpp -- the four plan objects of the reference (src/processor.rs: Forward :7-159, Inverse :231-341,
// Normalize :409-505, Onlyinverse :566-670) behind fwa_plan_create / fwa_plan_exec / fwa_plan_destroy.
//
// None of the reference's wgpu plumbing survives: a plan owns (or shares through the context's plan cache) its twiddle
// tables and scratch, exec only enqueues kernels on the caller's stream and allocates nothing.
#include <algorithm>
#include <chrono>
#include <new>

#include "internal.h"

using namespace fwa_int;

namespace fwa_int {

// Kernel families (FAM_* of schedule.h), each set up once per context, before the first plan that may launch one of its
// kernels -- and only then: a plan of n <= 4096 loads no k_small32<14 / 15>.  The order of the rows means nothing.
static const struct { uint32_t family; hipError_t (*setup)(); const char *name; } kFamilySetups[] = {
    {FAM_SMALL32, fwa::setup_small32_kernels, "small32"}, {FAM_1M, fwa::setup_1m_kernels, "1m"},
    {FAM_ROWS32, fwa::setup_rows32_kernels, "rows32"},    {FAM_COLSW, fwa::setup_colsw_kernels, "colsw"},
    {FAM_COLS32, fwa::setup_cols32_kernels, "cols32"},    {FAM_TILE, fwa::setup_tile_kernels, "tile"},
    {FAM_P1_GEN, fwa::setup_p1_gen_kernels, "p1_gen"},    {FAM_LAB_RING, fwa::setup_lab_1m_kernels, "lab_ring"},
};

// The families a plan may launch on its path.  A tiled plan counts every kernel that the keys "colsw", "rows32", "p1_gen" and
// "tile_ring" can select without a new setup ("factors" and "path" run setup_path again).
static uint32_t path_families(const fwa_plan *p)
{
    if (p->path == PATH_TILED) return families(p->lg, p->lf);
    if (p->path == PATH_SMALL) return p->n > 4096 ? FAM_SMALL32 : 0u;
    return p->path == PATH_TWOPASS_1M ? FAM_1M : p->path == PATH_RING_1M ? FAM_LAB_RING : 0u;
}

// Everything a plan needs for its path: kernel attributes (once per context), twiddle tables (shared through the
// context's plan cache) and, on the pipelined paths, the ring + internal streams with the default geometry.
// Two chains (pass A of one group beside pass C of another) pay off once each chain has a few groups to run; with fewer
// than 4 groups in all, the launches of the two chains only compete (2^20 x 32: 8.0 us per transform on two chains, 6.1
// on one; x 64: 6.2 against 6.5; 2^18 x 128: 1.68 against 1.51; profiles/round2/sweep_mid_batch_chains.jsonl).
int64_t default_chains(uint64_t batch, int64_t group)
{
    const uint64_t n_groups = group > 0 ? (batch + (uint64_t)group - 1) / (uint64_t)group : 0;
    return n_groups >= 4 ? 2 : 1;
}

int32_t setup_path(fwa_plan *p)
{
    fwa_ctx *ctx = p->ctx;
    const uint32_t fft_len = p->n;
    const uint32_t todo = path_families(p) & ~ctx->kernel_families;
    for (const auto &f : kFamilySetups) {
        if (!(todo & f.family)) continue;
        hipError_t e = f.setup();
        if (e != hipSuccess)
            return fail_hip(ctx, e, (std::string("hipFuncSetAttribute(max dynamic LDS), kernel family ") + f.name).c_str());
        ctx->kernel_families |= f.family;
    }
    // tables: shared by every plan of this (length, path, factorisation) on the context
    const uint32_t sig = p->lf[0] | (p->lf[1] << 8) | (p->lf[2] << 16);
    const auto key = std::make_tuple(fft_len, p->path == PATH_RING_1M ? (int64_t)PATH_TWOPASS_1M : p->path, sig);
    // The tables of the NEW path / factorisation are held locally and handed to the plan only once its pipeline has
    // been built: a failed re-tune (e.g. no memory for the new ring) leaves the plan with the tables of the factors it
    // keeps (the callers restore path and factors).
    std::shared_ptr<Tables> tb;
    auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        tb = it->second;
        ++ctx->n_table_hits;
    } else {
        tb = std::make_shared<Tables>();
        int32_t st = build_tables(ctx, fft_len, std::get<1>(key), p->lf, tb.get());
        if (st) return st;
        ++ctx->n_table_builds;
        ctx->tables.emplace(key, tb);
    }
    int32_t st = FWA_OK;
    if (p->path == PATH_TILED) {
        // the intermediate of a group of transforms lives in a ring slab of 128 MiB per chain (two chains = the
        // 256-MiB Infinity Cache; group sweep in profiles/round1/h_tiled_group_sweep.jsonl)
        const uint64_t per = (uint64_t)fft_len * sizeof(v2f);
        int64_t g = (int64_t)((128ull << 20) / per);
        if (g < 1) g = 1;
        st = build_pipeline(p, g, default_chains(p->batch, g));
    } else if (p->path == PATH_TWOPASS_1M) {
        st = build_pipeline(p, 16, default_chains(p->batch, 16));  // 16 transforms = 1024 tiles per launch
    } else if (p->path == PATH_RING_1M) {
        st = build_pipeline(p, 0, 0);
    }
    if (st) return st;
    p->tb = tb;
    return FWA_OK;
}

// processor.rs:153-157, :335-339, :664-668
static fwa_buf *result_buffer(fwa_plan *p) { return (p->lg % 2 == 0) ? p->src : p->second; }

// Block -> tile map (xcd_map, device_common.h) of a pipelined plan whose caller has not set "xcd_swizzle".  2^20 pipeline:
// XCD-contiguous tiles + adjacent tiles on the two residents of a CU (bit 2: + 4-8 % for launches that have the chip to
// themselves, + 0.6 % with two chains in flight: tile_1m.h xcd_block, profiles/round4/sweep_pair_map_two_chains.jsonl);
// tiled plans: per size, resolved with the passes (schedule.h).
uint32_t swizzle_default(const fwa_plan *p)
{
    if (p->path == PATH_TWOPASS_1M) return 5u;
    return p->path == PATH_TILED ? resolve_tiled(p->lg, p->lf, p->flags).xcd_swizzle : 0u;
}

// Run `body(group index, stream, chain index)` for every group, alternating over the plan's internal streams,
// forked from and joined back to the caller's stream with events.
template <class Body>
static int32_t run_groups(fwa_plan *plan, hipStream_t st, Body body)
{
    fwa_ctx *ctx = plan->ctx;
    const Pipeline &pl = plan->pipe;
    const uint64_t G = (uint64_t)pl.group, n_groups = (plan->batch + G - 1) / G;
    const size_t ns = pl.streams.size();
    if (plan->batch && !pl.ring)
        return fail(ctx, FWA_ERR_INVALID_ARG, "plan has no scratch ring (a failed re-tune?)");
    if (ns) {
        HIP_TRY(ctx, hipEventRecord(pl.fork, st));
        for (size_t i = 0; i < ns; ++i) HIP_TRY(ctx, hipStreamWaitEvent(pl.streams[i], pl.fork, 0));
    }
    hipError_t e = hipSuccess;
    for (uint64_t g = 0; g < n_groups && e == hipSuccess; ++g) {
        const size_t c = ns ? (size_t)(g % ns) : 0;
        const uint64_t cnt = (plan->batch - g * G < G) ? plan->batch - g * G : G;
        // laboratory knob "inject_launch_failure" (-1, never equal, in the product library: tuning.cpp)
        if (plan->inject_fail_group == (int64_t)g) { plan->inject_fail_group = -1; e = hipErrorLaunchFailure; break; }
        e = body(g, cnt, ns ? pl.streams[c] : st, c);
    }
    // Join the chains back to the caller's stream ALSO when a launch failed: the groups enqueued before the failure
    // keep running on the chains, and whatever the caller enqueues next on `st` (a copy of the partial result, the
    // free of the buffer) must be ordered behind them.
    hipError_t je = hipSuccess;
    for (size_t i = 0; i < ns; ++i) {
        hipError_t r = hipEventRecord(pl.done[i], pl.streams[i]);
        if (r == hipSuccess) r = hipStreamWaitEvent(st, pl.done[i], 0);
        if (r != hipSuccess) {
            // no event carries the order: the host waits for this chain instead, so that whatever is enqueued on `st`
            // after this call still comes behind it
            (void)hipGetLastError();
            (void)hipStreamSynchronize(pl.streams[i]);
            if (je == hipSuccess) je = r;
        }
    }
    plan->last_stream = st;
    plan->ran_on_stream = true;
    if (e != hipSuccess) return fail_hip(ctx, e, "kernel launch", FWA_ERR_LAUNCH);
    if (je != hipSuccess) return fail_hip(ctx, je, "hipEventRecord/hipStreamWaitEvent (join of the chain streams)");
    return FWA_OK;
}

// ---- the tiled path (PATH_TILED): n = N1*N2[*N3]; index n = (n1*N2 + n2)*N3 + n3, k = k1 + N1*(k2 + N2*k3) ----
//   pass A: FFT over n1 (columns, four-step twiddle W_n), user buffer -> ring slab
//   pass B: FFT over n2 per k1 (columns, twiddle W_{N2*N3}), in place in the slab            [three factors only]
//   pass C: FFT over the contiguous axis with the transposed store, slab -> result buffer
// Which kernel runs each pass is resolve_tiled's answer (schedule.h); the code below only fills in launch arguments.
// What the passes of one exec share: factor sizes, the block -> tile map and the slab layout pass A leaves for pass C.
struct TiledShape {
    uint64_t N, N1, N2, N3;
    bool three;
    uint32_t swizzle, ring_cw;   // xcd_map bits handed to every kernel; TiledSchedule::ring_cw
};

// One pass of a tiled exec: the resolved kernel, and every launch argument except the group's pointers and transform count.
// Built once per fwa_plan_exec by pass_a / pass_b / pass_c, immutable afterwards, called once per group.
struct TiledPass {
    TiledKernel kernel = TiledKernel::NONE;
    int dir = fwa::FWD;
    uint32_t lg_l = 0;                 // log2 of this pass's FFT length
    const v2f *tw = nullptr, *tw_lo = nullptr, *tw_hi = nullptr;
    const v2f *tw_inner = nullptr;     // k_p1_gen: its first-stage table in place of tw
    uint32_t pitch = 0;                // column kernels: columns of the n1 x pitch matrix
    uint32_t n1 = 0;                   // k_rows32: rows of the matrix
    uint64_t sb = 0;                   // elements between transforms, in and out
    float scale = 1.0f;
    uint32_t swizzle = 0, ring_cw = 0;
    fwa::TileArgs ta{};                // k_tile: complete except in / out
    hipError_t operator()(const v2f *in, v2f *out, uint64_t cnt, hipStream_t s) const
    {
        switch (kernel) {
            case TiledKernel::COLSW:
                return fwa::launch_colsw(dir, lg_l, ring_cw != 0, in, out, tw, tw_lo, tw_hi, pitch, sb, sb, (uint32_t)cnt,
                                         swizzle, s);
            case TiledKernel::COLS32:
                return fwa::launch_cols32(dir, lg_l, in, out, tw, tw_lo, tw_hi, pitch, sb, sb, (uint32_t)cnt, swizzle, s);
            case TiledKernel::P1_GEN:
                return fwa::launch_p1_gen(dir, in, out, tw_inner, tw_lo, tw_hi, pitch, sb, sb, (uint32_t)cnt, swizzle, s);
            case TiledKernel::ROWS32:
                return fwa::launch_rows32(dir, lg_l, in, out, tw, n1, sb, sb, (uint32_t)cnt, scale, swizzle, ring_cw, s);
            case TiledKernel::TILE_COLS:
            case TiledKernel::TILE_ROWS: {
                fwa::TileArgs t = ta;
                t.in = in; t.out = out;
                return fwa::launch_tile(dir, kernel == TiledKernel::TILE_COLS ? fwa::TILE_COLS : fwa::TILE_ROWS_T, lg_l, t, cnt, s);
            }
            case TiledKernel::NONE: break;
        }
        return hipSuccess;
    }
};

static TiledShape tiled_shape(const fwa_plan *p, const TiledSchedule &sc)
{
    const bool three = sc.passes == 3;
    return {p->n, 1ull << p->lf[0], 1ull << p->lf[1], three ? (1ull << p->lf[2]) : 1, three,
            p->xcd_swizzle < 0 ? sc.xcd_swizzle : (uint32_t)p->xcd_swizzle, sc.ring_cw};
}

// pass A: columns of length N1 at pitch N / N1, user buffer -> slab
static TiledPass pass_a(TiledKernel kernel, const fwa_plan *p, const TiledShape &sh, const Tables &tb, int dir)
{
    TiledPass ps;
    ps.kernel = kernel;
    ps.dir = dir; ps.lg_l = p->lf[0]; ps.sb = sh.N; ps.swizzle = sh.swizzle; ps.ring_cw = sh.ring_cw;
    ps.pitch = (uint32_t)(sh.N / sh.N1);
    ps.tw = tb.tw_l[0]; ps.tw_lo = tb.tw_lo1; ps.tw_hi = tb.tw_hi1; ps.tw_inner = tb.tw_inner;
    const uint32_t cw = fwa::TILE_CW;
    fwa::TileArgs &t = ps.ta;
    t.tw = tb.tw_l[0]; t.tw_lo = tb.tw_lo1; t.tw_hi = tb.tw_hi1;
    t.scale = 1.0f; t.cw = cw; t.role = fwa::ROLE_FIRST; t.xcd_swizzle = sh.swizzle;
    t.in_sb = t.out_sb = sh.N; t.in_s1 = t.out_s1 = 0; t.in_st = t.out_st = cw;
    t.pitch = sh.N / sh.N1; t.out_stride = 0; t.d1_count = 1; t.tile_count = (uint32_t)(sh.N / sh.N1 / cw);
    return ps;
}

// pass B (three factors): columns of length N2 at pitch N3 inside every k1-plane, in place in the slab
static TiledPass pass_b(TiledKernel kernel, const fwa_plan *p, const TiledShape &sh, const Tables &tb, int dir)
{
    TiledPass ps;
    if (!sh.three) return ps;   // kernel == NONE
    ps.kernel = kernel;
    ps.dir = dir; ps.lg_l = p->lf[1];
    const uint32_t cw = fwa::TILE_CW;
    fwa::TileArgs &t = ps.ta;
    t.tw = tb.tw_l[1]; t.tw_lo = tb.tw_lo_b; t.tw_hi = tb.tw_hi_b;
    t.scale = 1.0f; t.cw = cw; t.role = fwa::ROLE_MIDDLE; t.xcd_swizzle = sh.swizzle;
    t.in_sb = t.out_sb = sh.N; t.in_s1 = t.out_s1 = sh.N2 * sh.N3; t.in_st = t.out_st = cw;
    t.pitch = sh.N3; t.out_stride = 0; t.d1_count = (uint32_t)sh.N1; t.tile_count = (uint32_t)(sh.N3 / cw);
    return ps;
}

// pass C: rows of the last axis, adjacent k1 per tile, transposed store into the result buffer (+ the 1/n of Inverse)
static TiledPass pass_c(TiledKernel kernel, const fwa_plan *p, const TiledShape &sh, const Tables &tb, int dir, float scale)
{
    TiledPass ps;
    const uint32_t li = sh.three ? 2 : 1;
    ps.kernel = kernel;
    ps.dir = dir; ps.lg_l = p->lf[li]; ps.sb = sh.N; ps.scale = scale; ps.swizzle = sh.swizzle; ps.ring_cw = sh.ring_cw;
    ps.tw = tb.tw_l[li]; ps.n1 = (uint32_t)sh.N1;
    const uint32_t cw = fwa::TILE_CW;
    fwa::TileArgs &t = ps.ta;
    t.tw = tb.tw_l[li]; t.tw_lo = nullptr; t.tw_hi = nullptr;
    t.scale = scale; t.cw = cw; t.role = fwa::ROLE_LAST; t.xcd_swizzle = sh.swizzle;
    t.in_sb = t.out_sb = sh.N;
    t.pitch = sh.N / sh.N1;  // distance between the rows k1 and k1 + 1
    t.in_st = cw * (sh.N / sh.N1); t.out_st = cw; t.tile_count = (uint32_t)(sh.N1 / cw);
    if (sh.three) { t.d1_count = (uint32_t)sh.N2; t.in_s1 = sh.N3; t.out_s1 = sh.N1; t.out_stride = sh.N1 * sh.N2; }
    else { t.d1_count = 1; t.in_s1 = t.out_s1 = 0; t.out_stride = sh.N1; }
    return ps;
}

}  // namespace fwa_int

extern "C" {

// ---- plans ----------------------------------------------------------------
int32_t fwa_plan_destroy(fwa_plan *plan)
{
    if (!plan) return FWA_OK;
    (void)hipSetDevice(plan->ctx->device);
    // work of this plan may still be in flight on the caller's stream; the pooled ring must not be handed to the next
    // plan before it has drained (hipFree would have synchronised implicitly).  Only THIS plan's last exec is waited
    // for, through a marker on the stream that exec was enqueued on -- other streams and contexts keep running (a
    // device-wide synchronise here stalled them all and is illegal while any stream captures a graph).  An exec that
    // was captured into a graph enqueued nothing real: the plan must outlive the graphs that replay it.
    bool drained = true;
    if (plan->frozen && plan->pipe.ring) {
        hipEvent_t ev = nullptr;
        bool waited = false;
        // only a stream that is known to be alive can take the marker: the null stream, or a stream of this context's
        // own making that has not been destroyed (HIP does not validate stream handles); otherwise the device-wide
        // wait below
        bool alive = plan->last_stream == nullptr;
        for_each(plan->ctx->handles, H_STREAM, [&](const Handle *h) {
            const fwa_stream *s = static_cast<const fwa_stream *>(h);
            alive = alive || (s->owned && s->s == plan->last_stream);
        });
        if (plan->ran_on_stream && alive && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
            // everything this plan enqueued on its last caller stream precedes this marker
            if (hipEventRecord(ev, plan->last_stream) == hipSuccess) waited = hipEventSynchronize(ev) == hipSuccess;
            (void)hipEventDestroy(ev);
        }
        if (!waited) {
            (void)hipGetLastError();
            // the stream is gone or not ours (fwa_stream_wrap), or a laboratory persistent path
            drained = hipDeviceSynchronize() == hipSuccess;
            if (!drained) (void)hipGetLastError();
        }
    }
    // a ring that may still be in use is not pooled: it is freed, and hipFree synchronises
    release_pipeline(plan->ctx, plan->pipe, drained);
    if (plan->tw_half_private) (void)hipFree(plan->tw_half_private);
    if (plan->second_owned && plan->own_second.p) (void)hipFree(plan->own_second.p);
    delete plan;
    return FWA_OK;
}

int32_t fwa_plan_create(fwa_ctx *ctx, int32_t kind, uint32_t fft_len, fwa_buf *src, fwa_buf *src2_or_null,
                        fwa_plan **out)
{
    if (!out) return fail(ctx, FWA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx || !src) return fail(ctx, FWA_ERR_INVALID_ARG, "ctx/src is NULL");
    for (const fwa_buf *b : {(const fwa_buf *)src, (const fwa_buf *)src2_or_null}) {
        if (b && !b->ctx) return fail(ctx, FWA_ERR_INVALID_ARG, "a buffer belongs to a context that has been destroyed");
        if (b && b->ctx->device != ctx->device)
            return fail(ctx, FWA_ERR_INVALID_ARG, "a buffer lives on another device than the plan's context");
    }
    if (kind < FWA_FORWARD || kind > FWA_NORMALIZE) return fail(ctx, FWA_ERR_INVALID_ARG, "unknown plan kind");
    if (!is_pow2(fft_len)) return fail(ctx, FWA_ERR_INVALID_ARG, "fft_len must be a power of two >= 1");
    if (fft_len > (1u << 30)) return fail(ctx, FWA_ERR_UNSUPPORTED, "fft_len above 2^30 is not supported");
    const uint64_t tbytes = (uint64_t)fft_len * 8;
    if (src->bytes % tbytes != 0)
        return fail(ctx, FWA_ERR_INVALID_ARG, "buffer size is not a multiple of 8*fft_len bytes");
    const bool needs_src2 = (kind == FWA_INVERSE_UNSCALED || kind == FWA_NORMALIZE);
    if (needs_src2 && !src2_or_null)
        return fail(ctx, FWA_ERR_INVALID_ARG, "this plan kind needs a caller-supplied second buffer");
    if (!needs_src2 && src2_or_null)
        return fail(ctx, FWA_ERR_INVALID_ARG, "this plan kind owns its second buffer; pass NULL");
    if (src2_or_null && src2_or_null->bytes != src->bytes)
        return fail(ctx, FWA_ERR_INVALID_ARG, "second buffer must have the size of the first");
    if (src2_or_null && src->bytes) {
        // [p, p + bytes) of the two buffers: the same memory twice, or two views of one allocation that share a part
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(src->p), b0 = reinterpret_cast<uintptr_t>(src2_or_null->p);
        if (a0 == b0) return fail(ctx, FWA_ERR_INVALID_ARG, "the two buffers must be distinct");
        if (a0 < b0 + src2_or_null->bytes && b0 < a0 + src->bytes)
            return fail(ctx, FWA_ERR_INVALID_ARG, "the two buffers must not overlap");
    }
    if (reinterpret_cast<uintptr_t>(src->p) & 15)
        return fail(ctx, FWA_ERR_INVALID_ARG, "buffer must be 16-byte aligned");

    const auto t_begin = std::chrono::steady_clock::now();
    USE_DEVICE(ctx);
    fwa_plan *p = new (std::nothrow) fwa_plan;
    if (!p) return fail(ctx, FWA_ERR_OUT_OF_MEMORY, "host allocation failed");
    p->ctx = ctx; p->kind = kind; p->n = fft_len; p->lg = ilog2(fft_len);
    p->batch = src->bytes / tbytes;
    p->src = src; p->second = src2_or_null;

    int32_t st = FWA_OK;
    auto bail = [&](int32_t s) { fwa_plan_destroy(p); return s; };
    auto done = [&]() {
        ctx->last_plan_create_us =
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_begin).count();
        *out = p;
        return FWA_OK;
    };

    if (kind == FWA_NORMALIZE) {
        p->path = PATH_NORMALIZE;
        return done();
    }

    bool cw = false;
    p->path = choose_path(fft_len, p->batch, p->lf, &cw);
    p->flags.colsw = cw;

    // Forward/Inverse own their ping-pong partner (processor.rs:34-41,261-269).  It is only
    // materialised when the result must land there (odd log2 n) or the path ping-pongs.
    const bool odd = (p->lg & 1) != 0;
    const bool need_second = odd || p->path == PATH_R2_GLOBAL;
    if (!p->second && need_second && src->bytes) {
        hipError_t e = hipMalloc(&p->own_second.p, src->bytes);
        if (e != hipSuccess) return bail(fail_hip(ctx, e, "hipMalloc(second buffer)"));
        p->own_second.ctx = ctx; p->own_second.bytes = src->bytes; p->own_second.owned = false;
        p->second = &p->own_second;
        p->second_owned = true;
    } else if (!p->second) {
        // even log2 n on an in-place path: the reference would still own a buffer_b; we keep a
        // zero-sized handle so the result rule never dereferences NULL.
        p->own_second.ctx = ctx;
        p->second = &p->own_second;
    }

    st = setup_path(p);
    if (st) return bail(st);
    return done();
}

int32_t fwa_plan_exec(fwa_plan *plan, fwa_stream *stream, fwa_buf **result)
{
    if (!plan) return fail(nullptr, FWA_ERR_INVALID_ARG, "plan is NULL");
    fwa_ctx *ctx = plan->ctx;
    USE_DEVICE(ctx);
    hipStream_t st = raw(stream);
    plan->frozen = true;
    const uint64_t total = plan->batch * (uint64_t)plan->n;
    hipError_t e = hipSuccess;

    if (plan->kind == FWA_NORMALIZE) {
        // processor.rs:433-439: (a, b) = (buffer1, buffer2) if log2 n even else (buffer2, buffer1); returns b
        fwa_buf *a = (plan->lg % 2 == 0) ? plan->src : plan->second;
        fwa_buf *b = (plan->lg % 2 == 0) ? plan->second : plan->src;
        e = fwa::launch_scale(static_cast<const v2f *>(a->p), static_cast<v2f *>(b->p), total,
                              1.0f / (float)plan->n, st);
        if (e != hipSuccess) return fail_hip(ctx, e, "normalize launch", FWA_ERR_LAUNCH);
        if (result) *result = b;
        return FWA_OK;
    }

    const int dir = (plan->kind == FWA_FORWARD) ? fwa::FWD : fwa::INV;
    const float scale = (plan->kind == FWA_INVERSE_SCALED) ? 1.0f / (float)plan->n : 1.0f;  // ifft.wgsl:65-74
    fwa_buf *res = result_buffer(plan);
    if (result) *result = res;
    if (total == 0) return FWA_OK;
    v2f *a = static_cast<v2f *>(plan->src->p);
    v2f *b = static_cast<v2f *>(plan->second->p);
    v2f *out = static_cast<v2f *>(res->p);
    const Tables &tb = *plan->tb;
    const Pipeline &pl = plan->pipe;
    const uint64_t N = plan->n, G = (uint64_t)pl.group;

    switch (plan->path) {
        case PATH_IDENTITY:
            if (scale != 1.0f) e = fwa::launch_scale(a, a, total, scale, st);
            break;
        case PATH_SMALL:
            // laboratory kernels (A/B): the direct 16-point kernels (small_reg = 3, 16 <= n <= 4096), with the
            // wavefront-shuffle exchange at 32 / 64 / 128 (small_reg = 2, which leaves n >= 512 to k_small32)
            if (kLab && plan->small_reg != 1 && plan->n >= 16 && plan->n <= 4096 && (plan->small_reg == 3 || plan->n < 512)) {
                e = fwa::launch_small16(dir, a, out, tb.tw_half, plan->n, plan->batch, scale, plan->small_reg == 2, st);
                break;
            }
            if (plan->n <= 256)
                e = fwa::launch_chunk(dir, a, out, tb.tw_half, plan->n, plan->batch, scale, st);
            else
                e = fwa::launch_small32(dir, a, out, tb.tw_half, plan->n, plan->batch, scale, st);
            break;
        case PATH_R2_GLOBAL: {
            const v2f *tw = plan->tw_half_private ? plan->tw_half_private : tb.tw_half;
            for (uint32_t s = 0; s < plan->lg && e == hipSuccess; ++s) {
                const v2f *from = (s % 2 == 0) ? a : b;
                v2f *to = (s % 2 == 0) ? b : a;
                e = fwa::launch_r2_stage(dir, from, to, tw, plan->n, s, plan->batch, (s + 1 == plan->lg) ? scale : 1.0f,
                                         st);
            }
            break;
        }
        case PATH_TWOPASS_1M: {
            // in place at group granularity: 2^20 has even log2, the result buffer is src (processor.rs:153-157)
            const v2f *two = tb.tw_outer;
            const uint32_t swz = plan->xcd_swizzle < 0 ? swizzle_default(plan) : (uint32_t)plan->xcd_swizzle;
            return run_groups(plan, st, [&](uint64_t g, uint64_t cnt, hipStream_t s, size_t c) {
                // ring region of this chain: transform i -> slot i (ring_rotate > 1, laboratory: successive groups of a
                // chain walk through ring_rotate such regions)
                const uint64_t round = g / (pl.streams.empty() ? 1 : pl.streams.size());
                v2f *slab = pl.ring + (round % (uint64_t)plan->ring_rotate) *
                                          (uint64_t)pl.n_streams * G * N + (uint64_t)c * G * N;
                hipError_t le = fwa::launch_p1_1m(dir, a + g * G * N, slab, tb.tw_inner, two, (uint32_t)cnt, swz, s);
                if (le != hipSuccess) return le;
                return fwa::launch_p2_1m(dir, slab, out + g * G * N, tb.tw_inner, (uint32_t)cnt, scale, swz, s);
            });
        }
        case PATH_RING_1M: {
            if (!kLab) return fail(ctx, FWA_ERR_UNSUPPORTED, "plan path not implemented");
            if (!pl.ring || !pl.ctl)
                return fail(ctx, FWA_ERR_INVALID_ARG, "plan has no scratch ring (a failed re-tune?)");
            const uint64_t slots = (uint64_t)plan->ring_slots < plan->batch ? (uint64_t)plan->ring_slots : plan->batch;
            const uint64_t depth = (uint64_t)plan->depth < slots ? (uint64_t)plan->depth : (slots > 1 ? slots - 1 : 1);
            e = fwa::launch_ring_1m(dir, a, out, pl.ring, tb.tw_inner, tb.tw_outer, pl.ctl,
                                    (uint32_t)plan->batch,
                                    (uint32_t)depth, (uint32_t)(slots > depth ? slots : depth + 1),
                                        (uint32_t)plan->wgs, scale, st);
            break;
        }
        case PATH_TILED: {
            // Per group of transforms: pass A, user buffer -> ring slab; [pass B, in place in the slab]; pass C, slab ->
            // result buffer (src for even log2 n -- in place at group granularity -- else second).  The kernels are
            // resolved and the three passes built once per exec (TiledPass above: launch arguments, nothing on the heap)
            // and only receive the group's pointers here.
            const TiledSchedule sc = resolve_tiled(plan->lg, plan->lf, plan->flags);
            if (sc.a == TiledKernel::NONE || sc.c == TiledKernel::NONE || (sc.passes == 3 && sc.b == TiledKernel::NONE))
                return fail(ctx, FWA_ERR_UNSUPPORTED, "no kernel for a pass of these factors");
            const TiledShape shape = tiled_shape(plan, sc);
            const TiledPass pa = pass_a(sc.a, plan, shape, tb, dir), pb = pass_b(sc.b, plan, shape, tb, dir),
                            pc = pass_c(sc.c, plan, shape, tb, dir, scale);
            return run_groups(plan, st, [&](uint64_t g, uint64_t cnt, hipStream_t s, size_t c) {
                v2f *slab = pl.ring + (uint64_t)c * G * N;
                hipError_t le = pa(a + g * G * N, slab, cnt, s);
                if (le == hipSuccess && pb.kernel != TiledKernel::NONE) le = pb(slab, slab, cnt, s);
                if (le == hipSuccess) le = pc(slab, out + g * G * N, cnt, s);
                return le;
            });
        }
        default:
            return fail(ctx, FWA_ERR_UNSUPPORTED, "plan path not implemented");
    }
    if (e != hipSuccess) return fail_hip(ctx, e, "kernel launch", FWA_ERR_LAUNCH);
    return FWA_OK;
}

int32_t fwa_describe_path(uint32_t fft_len, int32_t *path, uint32_t log2_factors[3])
{
    if (!path || !log2_factors) return fail(nullptr, FWA_ERR_INVALID_ARG, "NULL argument");
    if (!is_pow2(fft_len)) return fail(nullptr, FWA_ERR_INVALID_ARG, "fft_len must be a power of two >= 1");
    if (fft_len > (1u << 30)) return fail(nullptr, FWA_ERR_UNSUPPORTED, "fft_len above 2^30 is not supported");
    *path = (int32_t)choose_path(fft_len, ~0ull, log2_factors);
    return FWA_OK;
}

}  // extern "C"
