// tuning.cpp -- fwa_plan_get_i64 / fwa_plan_set_i64: what a plan chose at creation, and the keys that re-tune it
// before its first exec.  No key changes what a plan computes (tests/test_gpu_parity.py: every alternative is
// bit-identical where it shares arithmetic); the reference has no counterpart (one radix-2 loop, src/kernel/fft4.wgsl).
#include "internal.h"

using namespace fwa_int;

// One re-tune: `change` assigns to the choice a plan can re-tune -- path, factors and the laboratory's ring_rotate, depth
// and ring_slots -- then the plan is set up again (setup_path: tables + pipeline with the default geometry) or only its
// pipeline rebuilt with the geometry it has.  Both swap their result in only once it is complete, so putting the choice
// back is all a failure needs: the plan is then exactly as it was.
template <class Change>
static int32_t retune(fwa_plan *p, bool new_path, Change change)
{
    const int64_t old[4] = {p->path, p->ring_rotate, p->depth, p->ring_slots};
    const uint32_t old_lf[3] = {p->lf[0], p->lf[1], p->lf[2]};
    change();
    const int32_t st = new_path ? setup_path(p) : build_pipeline(p, p->pipe.group, p->pipe.n_streams);
    if (st) {
        p->path = old[0]; p->ring_rotate = old[1]; p->depth = old[2]; p->ring_slots = old[3];
        for (int i = 0; i < 3; ++i) p->lf[i] = old_lf[i];
    }
    return st;
}

extern "C" {

int32_t fwa_plan_get_i64(const fwa_plan *plan, const char *key, int64_t *value)
{
    if (!plan || !key || !value) return fail(plan ? plan->ctx : nullptr, FWA_ERR_INVALID_ARG, "NULL argument");
    const std::string k(key);
    const Pipeline &pl = plan->pipe;
    const int64_t ng = pl.group ? (int64_t)((plan->batch + pl.group - 1) / pl.group) : 0;
    if (k == "batch") *value = (int64_t)plan->batch;
    else if (k == "fft_len") *value = plan->n;
    else if (k == "path") *value = plan->path;
    else if (k == "group") *value = pl.group;
    else if (k == "streams") *value = pl.n_streams;
    else if (k == "tile_w") *value = 16;   // one tile width ships (kept as a key: bench lines of every round carry it)
    else if (k == "xcd_swizzle") *value = plan->xcd_swizzle < 0 ? (int64_t)swizzle_default(plan) : plan->xcd_swizzle;
    else if (k == "depth") *value = plan->depth;
    else if (k == "ring_slots") *value = plan->ring_slots;
    else if (k == "wgs") *value = plan->wgs;
    else if (k == "device_error") {
        // bounded-spin timeout flag of the persistent kernel (0 in every healthy run); synchronises the device
        *value = 0;
        if (pl.ctl) {
            uint32_t w = 0;
            HIP_TRY(plan->ctx, hipDeviceSynchronize());
            HIP_TRY(plan->ctx, hipMemcpy(&w, pl.ctl + 1, sizeof(w), hipMemcpyDeviceToHost));
            *value = w;
        }
    }
    else if (k == "small_reg") *value = plan->small_reg;
    else if (k == "p1_gen") *value = plan->flags.p1_gen;
    else if (k == "rows32") *value = plan->flags.rows32;
    else if (k == "colsw") *value = plan->flags.colsw;
    else if (k == "tile_ring") *value = plan->flags.tile_ring;
    else if (k == "ring_rotate") *value = plan->ring_rotate;
    else if (k == "factors") *value = plan->lf[0] | (plan->lf[1] << 8) | (plan->lf[2] << 16);
    // other holders: cache + plans
    else if (k == "tables_shared") *value = plan->tb ? (int64_t)plan->tb.use_count() - 1 : 0;
    else if (k == "scratch_bytes")
        *value = (int64_t)(pl.ring_bytes + pl.ctl_bytes) + (plan->second_owned ? (int64_t)plan->own_second.bytes : 0);
    else if (k == "launches_per_exec") {
        switch (plan->path) {
            case PATH_TWOPASS_1M: *value = 2 * ng; break;
            case PATH_RING_1M: *value = 1; break;
            case PATH_TILED: *value = resolve_tiled(plan->lg, plan->lf, plan->flags).passes * ng; break;
            case PATH_R2_GLOBAL: *value = plan->lg; break;
            case PATH_IDENTITY: *value = 0; break;   // n = 1: also the scaled inverse's 1/n is 1, and exec launches nothing
            default: *value = 1;
        }
    } else return fail(plan->ctx, FWA_ERR_INVALID_ARG, "unknown key: " + k);
    return FWA_OK;
}

int32_t fwa_plan_set_i64(fwa_plan *plan, const char *key, int64_t value)
{
    if (!plan || !key) return fail(plan ? plan->ctx : nullptr, FWA_ERR_INVALID_ARG, "NULL argument");
    if (plan->frozen) return fail(plan->ctx, FWA_ERR_INVALID_ARG, "plan tunables are locked after the first exec");
    fwa_ctx *ctx = plan->ctx;
    USE_DEVICE(ctx);
    const std::string k(key);
    if (k == "group" || k == "streams") {
        if (!is_pipelined(plan->path))
            return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to the pipelined paths (2^20 two-pass, tiled)");
        if (value < 1 || value > (k == "streams" ? 16 : 4096))
            return fail(ctx, FWA_ERR_INVALID_ARG, "value out of range");
        return build_pipeline(plan, k == "group" ? value : plan->pipe.group, k == "streams" ? value : plan->pipe.n_streams);
    }
    if (k == "inject_launch_failure") {
        // laboratory: the launch of group `value` fails once (nothing is enqueued for it): the error path of run_groups
        if (!kLab)
            return fail(ctx, FWA_ERR_UNSUPPORTED,
                        "inject_launch_failure is a laboratory knob (libfft_wgpu_amd_lab.so)");
        if (!is_pipelined(plan->path))
            return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to the pipelined paths");
        plan->inject_fail_group = value;
        return FWA_OK;
    }
    if (k == "ring_rotate") {
        if (!kLab) return fail(ctx, FWA_ERR_UNSUPPORTED, "ring_rotate is a laboratory knob (libfft_wgpu_amd_lab.so)");
        if (plan->path != PATH_TWOPASS_1M)
            return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to the 2^20 two-pass path");
        if (value < 1 || value > 64) return fail(ctx, FWA_ERR_INVALID_ARG, "value out of range");
        return retune(plan, false, [&] { plan->ring_rotate = value; });
    }
    if (k == "tile_w") {
        if (plan->path != PATH_TWOPASS_1M)
            return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to the 2^20 two-pass path");
        if (value != 16) return fail(ctx, FWA_ERR_UNSUPPORTED, "tile_w is 16 (the 32-column tile left the tree in round 6)");
        return FWA_OK;
    }
    if (k == "depth" || k == "ring_slots" || k == "wgs") {
        if (!kLab) return fail(ctx, FWA_ERR_UNSUPPORTED, "key belongs to a laboratory path (libfft_wgpu_amd_lab.so)");
        if (plan->path != PATH_RING_1M)
            return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to the persistent 2^20 path");
        if (value < 1 || value > 65536) return fail(ctx, FWA_ERR_INVALID_ARG, "value out of range");
        if (k == "wgs") { plan->wgs = value; return FWA_OK; }
        if (k == "depth")
            return retune(plan, false, [&] { plan->depth = value; if (plan->ring_slots < value + 1) plan->ring_slots = value + 1; });
        if (value < plan->depth + 1) return fail(ctx, FWA_ERR_INVALID_ARG, "ring_slots must exceed depth");
        return retune(plan, false, [&] { plan->ring_slots = value; });
    }
    if (k == "xcd_swizzle") {
        if (!is_pipelined(plan->path))
            return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to the pipelined paths");
        plan->xcd_swizzle = value & 7;
        return FWA_OK;
    }
    if (k == "factors") {
        // re-factorise a multi-pass plan: value = log2(N1) | log2(N2) << 8 | log2(N3) << 16 (N3 = 0: two passes), every
        // factor a length its pass has a kernel for, product n.  A tuning knob: every factorisation computes the same transform.
        if (!is_pipelined(plan->path)) return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to multi-pass plans");
        const uint32_t f[3] = {(uint32_t)value & 255u, (uint32_t)(value >> 8) & 255u, (uint32_t)(value >> 16) & 255u};
        if (!factors_valid(plan->lg, f))
            return fail(ctx, FWA_ERR_INVALID_ARG, "every factor must be 2^6..2^10 (2^11: first; 2^11, 2^12: second of two)");
        if (f[0] + f[1] + f[2] != plan->lg || (value >> 24))
            return fail(ctx, FWA_ERR_INVALID_ARG, "factors do not multiply to fft_len");
        return retune(plan, true, [&] {
            plan->path = PATH_TILED;
            plan->lf[0] = f[0]; plan->lf[1] = f[1]; plan->lf[2] = f[2];
        });
    }
    if (k == "p1_gen" || k == "rows32" || k == "colsw" || k == "tile_ring") {
        if (plan->path != PATH_TILED) return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to tiled plans");
        TiledFlags &fl = plan->flags;
        int64_t &flag = k == "p1_gen" ? fl.p1_gen : k == "rows32" ? fl.rows32 : k == "colsw" ? fl.colsw : fl.tile_ring;
        flag = value != 0;
        return FWA_OK;
    }
    if (k == "small_reg") {
        if (plan->path != PATH_SMALL) return fail(ctx, FWA_ERR_UNSUPPORTED, "key only applies to n <= 32768");
        if (value != 1 && !kLab)
            return fail(ctx, FWA_ERR_UNSUPPORTED, "small_reg != 1 selects laboratory kernels (libfft_wgpu_amd_lab.so)");
        // 1: k_chunk (2 .. 256) and k_small32 (from 512), the default; 3: the direct-addressing kernel k_small16 at
        // 16 .. 4096 (A/B); 2: as 3 up to 256 with the wavefront-shuffle exchange at n = 32 / 64 / 128
        if (value < 1 || value > 3) return fail(ctx, FWA_ERR_INVALID_ARG, "small_reg is 1, 2 or 3");
        plan->small_reg = value;
        return FWA_OK;
    }
    if (k == "path") {
        if (plan->kind == FWA_NORMALIZE) return fail(ctx, FWA_ERR_UNSUPPORTED, "normalize has one path");
        if (value == plan->path) return FWA_OK;
        if (value == PATH_RING_1M && !kLab)
            return fail(ctx, FWA_ERR_UNSUPPORTED, "path 5 is a laboratory path (libfft_wgpu_amd_lab.so)");
        if ((value == PATH_RING_1M || value == PATH_TWOPASS_1M)
            && (plan->path == PATH_RING_1M || plan->path == PATH_TWOPASS_1M)) {
            // the two forms of the 2^20 pipeline: per-group launches with a large ring, or one persistent launch (whose
            // control words go with its pipeline when the plan switches back)
            return retune(plan, true, [&] { plan->path = value; });
        }
        if (value == PATH_R2_GLOBAL && plan->n >= 2) {
            // force the literal reference recurrence (one launch per stage, kernel/fft.wgsl:27-62)
            if (!plan->tb->tw_half && !plan->tw_half_private) {
                int32_t st = upload_half_table(ctx, plan->n, &plan->tw_half_private);
                if (st) return st;
            }
            if (!plan->second->p && plan->src->bytes) {
                if (plan->second != &plan->own_second) return fail(ctx, FWA_ERR_INVALID_ARG, "second buffer missing");
                hipError_t e = hipMalloc(&plan->own_second.p, plan->src->bytes);
                if (e != hipSuccess) return fail_hip(ctx, e, "hipMalloc(second buffer)");
                plan->own_second.bytes = plan->src->bytes;
                plan->second_owned = true;
            }
            release_pipeline(ctx, plan->pipe, true);
            plan->path = PATH_R2_GLOBAL;
            return FWA_OK;
        }
        return fail(ctx, FWA_ERR_UNSUPPORTED,
                    "only path = 2 (the literal radix-2 recurrence) or, at n = 2^20, 1 / 5 can be set");
    }
    return fail(ctx, FWA_ERR_INVALID_ARG, "unknown key: " + k);
}

}  // extern "C"
