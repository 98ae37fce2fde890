// host_faults.cpp -- the library's host layer (fft_wgpu_amd/csrc/*.cpp and the five side-library hosts, compiled as they
// are) linked against a simulated HIP runtime (fake_hip.cpp), simulated launchers (fake_kernels.cpp) and, through the
// dlopen of comm.cpp, a simulated RCCL (fake_rccl.cpp): no device, no Python, no threads.  Scenarios are plain functions
// over the public C ABI (one over the C++ mirror's Comm) that check every status.
//
//   --selftest   the fakes are misused directly; every misuse must be reported as its own kind of violation
//   --clean      every scenario with nothing armed: no violation, launches per exec as the plan says, exec allocates
//                nothing, nothing left alive
//   --geometry   tiled and pipelined plans of every log2 n = 16 .. 30 x batch x group x streams: one exec each under the
//                bounds / written / hazard checks (pure arithmetic: device memory is address space only); then the framed plans
//                of every n = 2 .. 4096 x hop x signal length x signals
//   --faults     every scenario on n <= 2^20 once per injectable call of its clean run, that call failing: what the header
//                promises after a failure must hold (see failed() and the wrappers below), then the scenario goes on to its
//                end, where every later exec must record what the clean run recorded.  A collective of a communicator that
//                fails is given up (the header: fatal for the communicator) and everything is destroyed
//   --stub       against a librccl.so.1 without ncclRecv: the fwa_comm_* calls answer FWA_ERR_UNSUPPORTED and name the symbol
// --clean, --faults and --stub need the simulated RCCL in LD_LIBRARY_PATH and refuse to run with any other librccl.so.1.
// The last line of output is the summary the test asserts; stderr stays empty unless something is wrong.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../fft_wgpu_amd/csrc/internal.h"  // fwa_stream::s only: which runtime stream a handle stands for
#include "../../include/fft_wgpu_amd.h"
#include "../../include/fft_wgpu_amd_2d.h"
#include "../../include/fft_wgpu_amd_conv.h"
#include "../../include/fft_wgpu_amd_real.h"
#include "../../include/fft_wgpu_amd_stft.h"
#include "../../include/fft_wgpu_amd_strided.h"
#include "../../fft_wgpu_amd/stft/stft_kernels.h"  // the self-test calls the simulated framed launcher directly
#pragma clang diagnostic push  // (a product header: not held to the warnings of the simulator's own files)
#pragma clang diagnostic ignored "-Wunused-private-field"
#include "../../include/fft_wgpu.hpp"              // fft_wgpu::Comm: one scenario drives the ranks through the C++ mirror
#pragma clang diagnostic pop
#include "fake_hip.h"

extern "C" {  // fake_rccl.cpp, for the self-test: the scenarios reach these through comm.cpp and librccl.so.1 only
ncclResult_t fake_rccl_get_unique_id(ncclUniqueId *id);
ncclResult_t fake_rccl_comm_init_rank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank);
ncclResult_t fake_rccl_comm_destroy(ncclComm_t comm);
ncclResult_t fake_rccl_group_start(void);
ncclResult_t fake_rccl_group_end(void);
ncclResult_t fake_rccl_send(const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream);
ncclResult_t fake_rccl_recv(void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream);
}

namespace {

using sim::V_CHECK;

struct Abort {};   // thrown by the harness (never across the C ABI) when a scenario cannot go on
struct GiveUp {};  // a collective failed by injection: the scenario destroys everything (fatal for the communicator)

// HSA_ENABLE_IPC_MODE_LEGACY as the program set it for this run: 0 = unset, 1 = "1", 2 = "0"
int g_ipc_mode = 0;
void set_ipc_mode(int mode)
{
    g_ipc_mode = mode;
    if (mode == 0) (void)unsetenv("HSA_ENABLE_IPC_MODE_LEGACY");
    else (void)setenv("HSA_ENABLE_IPC_MODE_LEGACY", mode == 1 ? "1" : "0", 1);
}

struct Run {
    bool tolerant = false;
    bool failure_seen = false;
    bool gave_up = false;                                // a collective failed and the scenario went straight to its teardown
    std::vector<std::vector<std::string>> execs;         // what every successful exec recorded, in order
    std::string name;
};
Run *R = nullptr;

void check(bool ok, const std::string &what)
{
    if (!ok) sim::violation(V_CHECK, R->name + ": " + what);
}

// "The error string names the failing step": it holds the failing function's name, or -- beside the name of the injected error
// code -- the word the library uses for that class of step: a launcher is a "launch", a kernel-family setup is
// "hipFuncSetAttribute", and the overlap check of a new stream (ctx_streams.cpp: a dozen event, wait and spin-launch calls
// reported as one step) is "stream setup".  The error code alone does not pass.
bool names_step(const std::string &msg, const std::string &fn, const char *error_name)
{
    if (msg.find(fn) != std::string::npos) return true;
    if (msg.find(error_name) == std::string::npos) return false;
    if (fn.compare(0, 7, "launch_") == 0 && msg.find("launch") != std::string::npos) return true;
    if (fn.compare(0, 6, "setup_") == 0 && msg.find("hipFuncSetAttribute") != std::string::npos) return true;
    return msg.compare(0, 12, "stream setup") == 0;
}

// A non-zero status.  Strict runs have none.  A tolerant run has at most one, caused by the armed call: the status is one of
// the header's codes and the error string names what failed.  true = the caller repeats the call, which must succeed.
bool failed(int32_t st, const char *what, const fwa_ctx *ctx)
{
    if (st == FWA_OK) return false;
    const std::string on_ctx = ctx ? fwa_last_error_string(ctx) : "", on_thread = fwa_last_error_string(nullptr);
    if (!R->tolerant || !sim::fired() || R->failure_seen) {
        check(false, std::string(what) + " returned " + std::to_string(st) + " (" + on_ctx + " / " + on_thread + ")");
        throw Abort();
    }
    R->failure_seen = true;
    check(st >= FWA_ERR_INVALID_ARG && st <= FWA_ERR_UNSUPPORTED, std::string(what) + ": status " + std::to_string(st) + " is no fwa_status");
    bool named = false;
    for (const std::string &s : {on_ctx, on_thread}) named = named || names_step(s, sim::fired_name(), hipGetErrorName(sim::fired_error()));
    check(named, std::string(what) + " failed at " + sim::fired_name() + " but the error string is '" + on_ctx + "' / '" + on_thread + "'");
    if (sim::fired_name().compare(0, 4, "nccl") == 0) {  // an RCCL failure: FWA_ERR_HIP, and the hint unless the variable is "0"
        check(st == FWA_ERR_HIP, std::string(what) + " failed at " + sim::fired_name() + " with status " + std::to_string(st) + ", not FWA_ERR_HIP");
        const bool hint = (on_ctx + on_thread).find("HSA_ENABLE_IPC_MODE_LEGACY") != std::string::npos;
        const bool want = g_ipc_mode != 2 && sim::fired_name() != "ncclGetUniqueId";  // (no peer is mapped for an id)
        check(hint == want, std::string(what) + " failed at " + sim::fired_name() + " with the variable " + (g_ipc_mode == 0 ? "unset" : g_ipc_mode == 1 ? "\"1\"" : "\"0\"") +
                                (hint ? ": the error string carries the hint" : ": the error string lacks the hint") + " ('" + on_ctx + "' / '" + on_thread + "')");
    }
    return true;
}

template <class F>
void call(const char *what, const fwa_ctx *ctx, F f)
{
    if (!failed(f(), what, ctx)) return;
    const int32_t st = f();
    if (st != FWA_OK) {
        check(false, std::string(what) + " repeated with nothing armed returned " + std::to_string(st));
        throw Abort();
    }
}
// f() writes *out; a failed create leaves it null
template <class T, class F>
void create(const char *what, const fwa_ctx *ctx, T **out, F f)
{
    *out = reinterpret_cast<T *>(uintptr_t(16));
    if (failed(f(), what, ctx)) {
        check(*out == nullptr, std::string(what) + " failed and left *out set");
        const int32_t st = f();
        if (st != FWA_OK) {
            check(false, std::string(what) + " repeated with nothing armed returned " + std::to_string(st));
            throw Abort();
        }
    }
    if (!*out || *out == reinterpret_cast<T *>(uintptr_t(16))) { check(false, std::string(what) + " succeeded without an object"); throw Abort(); }
}
// a call whose contract is the status `want`
template <class F>
void expect(const char *what, const fwa_ctx *ctx, int32_t want, F f)
{
    int32_t st = f();
    if (st != want && failed(st, what, ctx)) st = f();
    check(st == want, std::string(what) + " returned " + std::to_string(st) + ", the header says " + std::to_string(want));
}

const char *const kPlanKeys[] = {"batch", "fft_len", "path", "group", "streams", "tile_w", "xcd_swizzle", "depth", "ring_slots", "wgs",
                                 "small_reg", "p1_gen", "rows32", "colsw", "tile_ring", "ring_rotate", "factors", "tables_shared",
                                 "scratch_bytes", "launches_per_exec"};
std::vector<int64_t> plan_state(const fwa_plan *p)
{
    std::vector<int64_t> v;
    for (const char *k : kPlanKeys) {
        int64_t x = -1;
        check(fwa_plan_get_i64(p, k, &x) == FWA_OK, std::string("fwa_plan_get_i64 ") + k);
        v.push_back(x);
    }
    return v;
}
void print_counters(const fwa_ctx *ctx, const char *after)
{
    std::printf("    counters after a failed %s:", after);
    for (const char *k : {"table_builds", "table_cache_hits", "ring_allocs", "ring_reuses", "pooled_ring_bytes", "chain_streams"}) {
        int64_t x = 0;
        (void)fwa_ctx_get_i64(ctx, k, &x);
        std::printf(" %s=%lld", k, (long long)x);
    }
    std::printf("\n");
}
bool g_verbose = false;

// a failed set leaves every key as it was
void set(fwa_plan *p, const fwa_ctx *ctx, const char *key, int64_t value)
{
    const std::vector<int64_t> before = plan_state(p);
    const std::string what = std::string("fwa_plan_set_i64(") + key + ", " + std::to_string(value) + ")";
    if (!failed(fwa_plan_set_i64(p, key, value), what.c_str(), ctx)) return;
    const std::vector<int64_t> after = plan_state(p);
    for (size_t i = 0; i < before.size(); ++i)
        check(before[i] == after[i], what + " failed and changed " + kPlanKeys[i] + " from " + std::to_string(before[i]) + " to " + std::to_string(after[i]));
    print_counters(ctx, what.c_str());  // printed, not asserted: a failed re-tune may have built tables or spent a pooled ring
    const int32_t st = fwa_plan_set_i64(p, key, value);
    if (st != FWA_OK) {
        check(false, what + " repeated with nothing armed returned " + std::to_string(st) + " (" + fwa_last_error_string(ctx) + ")");
        throw Abort();
    }
}

// what an exec recorded, free of addresses: launcher, caller's stream or the i-th internal one, every range as offset + length
// inside an allocation of a size
std::vector<std::string> signature(size_t first, hipStream_t caller)
{
    std::vector<std::string> sig;
    std::map<hipStream_t, int> internal;
    const std::vector<sim::Op> &ops = sim::ops();
    for (size_t i = first; i < ops.size(); ++i) {
        const sim::Op &o = ops[i];
        std::string s = o.name;
        if (o.stream == caller) s += " @caller";
        else {
            if (!internal.count(o.stream)) { const int k = (int)internal.size(); internal[o.stream] = k; }
            s += " @chain" + std::to_string(internal[o.stream]);
        }
        for (int w = 0; w < 2; ++w)
            for (const sim::Range &r : w ? o.writes : o.reads) {
                uint64_t base = 0, size = 0;
                (void)sim::locate(r.lo, &base, &size);
                s += (w ? " w:" : " r:") + std::to_string(r.lo - base) + "+" + std::to_string(r.hi - r.lo) + "/" + std::to_string(size);
            }
        sig.push_back(s);
    }
    return sig;
}

// One exec through `run` (fwa_plan_exec or a side library's), on `stream`, of a plan that says `launches` per exec.  After a
// failure: everything the exec enqueued anywhere is ordered behind a marker recorded next on the caller's stream; repeated, it
// succeeds.  Always: as many launches as the plan says, nothing allocated, no stream or event created.
void exec_checked(const char *what, const fwa_ctx *ctx, fwa_stream *stream, int64_t launches, const std::function<int32_t()> &run)
{
    const hipStream_t raw = stream ? stream->s : nullptr;
    size_t first = sim::ops().size();
    sim::Counters c0 = sim::counters();
    if (failed(run(), what, ctx)) {
        std::string which;
        check(sim::all_before_marker(first, raw, &which), std::string(what) + " failed and left " + which + " unordered before the caller's stream");
        first = sim::ops().size();
        c0 = sim::counters();
        const int32_t st = run();
        if (st != FWA_OK) {
            check(false, std::string(what) + " repeated with nothing armed returned " + std::to_string(st));
            throw Abort();
        }
    }
    const sim::Counters c1 = sim::counters();
    check(c0.mallocs == c1.mallocs && c0.host_mallocs == c1.host_mallocs, std::string(what) + " allocated memory");
    check(c0.streams_created == c1.streams_created && c0.events_created == c1.events_created, std::string(what) + " created a stream or an event");
    int64_t n = 0;
    for (size_t i = first; i < sim::ops().size(); ++i) n += sim::ops()[i].launch;
    check(n == launches, std::string(what) + " recorded " + std::to_string(n) + " launches, launches_per_exec is " + std::to_string(launches));
    R->execs.push_back(signature(first, raw));
}
void exec(fwa_plan *p, const fwa_ctx *ctx, fwa_stream *stream, fwa_buf **result = nullptr)
{
    int64_t launches = -1;
    check(fwa_plan_get_i64(p, "launches_per_exec", &launches) == FWA_OK, "launches_per_exec");
    exec_checked("fwa_plan_exec", ctx, stream, launches, [&] { return fwa_plan_exec(p, stream, result); });
}

// ---- building blocks ----
fwa_ctx *new_ctx(int device = 0)
{
    fwa_ctx *ctx = nullptr;
    create("fwa_ctx_create", nullptr, &ctx, [&] { return fwa_ctx_create(device, &ctx); });
    return ctx;
}
fwa_stream *new_stream(fwa_ctx *ctx)
{
    fwa_stream *s = nullptr;
    create("fwa_stream_create", ctx, &s, [&] { return fwa_stream_create(ctx, &s); });
    return s;
}
fwa_buf *new_buf(fwa_ctx *ctx, uint64_t bytes)
{
    fwa_buf *b = nullptr;
    create("fwa_buf_alloc", ctx, &b, [&] { return fwa_buf_alloc(ctx, bytes, &b); });
    return b;
}
// "the scenario uploads the source": from host memory up to 1 MiB, generated on the device above that; then the device is idle
void fill(fwa_ctx *ctx, fwa_buf *b, uint32_t n)
{
    const uint64_t bytes = fwa_buf_size(b);
    if (bytes <= (1u << 20)) {
        std::vector<char> host(bytes, 1);
        call("fwa_buf_upload", ctx, [&] { return fwa_buf_upload(b, 0, host.data(), bytes, nullptr); });
    } else {
        call("fwa_fill_synthetic", ctx, [&] { return fwa_fill_synthetic(b, 7, 0, n, 1.0f, nullptr); });
    }
    call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
}
fwa_buf *new_src(fwa_ctx *ctx, uint64_t n, uint64_t batch)
{
    fwa_buf *b = new_buf(ctx, n * batch * 8);
    fill(ctx, b, (uint32_t)n);
    return b;
}
fwa_plan *new_plan(fwa_ctx *ctx, int32_t kind, uint32_t n, fwa_buf *src, fwa_buf *src2)
{
    fwa_plan *p = nullptr;
    create("fwa_plan_create", ctx, &p, [&] { return fwa_plan_create(ctx, kind, n, src, src2, &p); });
    return p;
}
void peek(fwa_ctx *ctx, fwa_buf *b, fwa_stream *s)  // 64 bytes of a result, synchronously
{
    char host[64];
    const uint64_t bytes = fwa_buf_size(b) < 64 ? fwa_buf_size(b) : 64;
    call("fwa_buf_download", ctx, [&] { return fwa_buf_download(host, b, 0, bytes, s); });
}
int64_t ctx_get(const fwa_ctx *ctx, const char *key)
{
    int64_t v = -1;
    check(fwa_ctx_get_i64(ctx, key, &v) == FWA_OK, std::string("fwa_ctx_get_i64 ") + key);
    return v;
}
int64_t plan_get(const fwa_plan *p, const char *key)
{
    int64_t v = -1;
    check(fwa_plan_get_i64(p, key, &v) == FWA_OK, std::string("fwa_plan_get_i64 ") + key);
    return v;
}
hipStream_t raw_stream()  // a stream of the caller's own making, for fwa_stream_wrap
{
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    check(e == hipSuccess, "hipStreamCreateWithFlags of the scenario");
    return s;
}
void raw_stream_destroy(hipStream_t s)
{
    if (hipStreamDestroy(s) != hipSuccess) (void)hipGetLastError();
}

// ---- scenarios ----
struct Scenario { std::string name; uint64_t max_n; std::function<void()> run; };
std::vector<Scenario> g_scenarios;
void add(const std::string &name, uint64_t max_n, std::function<void()> f) { g_scenarios.push_back({name, max_n, std::move(f)}); }

// create, exec twice, read a little of the result, destroy
void life_cycle(int32_t kind, uint32_t n, uint64_t batch)
{
    fwa_ctx *ctx = new_ctx();
    fwa_stream *s = new_stream(ctx);
    fwa_buf *src = new_src(ctx, n, batch), *src2 = nullptr;
    if (kind == FWA_INVERSE_UNSCALED || kind == FWA_NORMALIZE) src2 = new_src(ctx, n, batch);
    fwa_plan *p = new_plan(ctx, kind, n, src, src2);
    fwa_buf *res = nullptr;
    exec(p, ctx, s, &res);
    exec(p, ctx, s, &res);
    check(res != nullptr, "exec returned no result buffer");
    peek(ctx, res, s);
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p); });
    call("fwa_buf_free", ctx, [&] { return fwa_buf_free(src); });
    call("fwa_buf_free", ctx, [&] { return fwa_buf_free(src2); });
    call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}

// a plan on (n, batch), a list of (key, value) re-tunes, one exec
void retune(int32_t kind, uint32_t n, uint64_t batch, const std::vector<std::pair<const char *, int64_t>> &steps)
{
    fwa_ctx *ctx = new_ctx();
    fwa_stream *s = new_stream(ctx);
    fwa_buf *src = new_src(ctx, n, batch), *src2 = kind == FWA_INVERSE_UNSCALED ? new_src(ctx, n, batch) : nullptr;
    fwa_plan *p = new_plan(ctx, kind, n, src, src2);
    for (const auto &kv : steps) {
        int64_t v = kv.second;
        if (!std::strcmp(kv.first, "factors") && v < 0)  // a second factorisation of 2^16: whichever the plan does not have
            v = plan_get(p, "factors") == (8 | (8 << 8)) ? (10 | (6 << 8)) : (8 | (8 << 8));
        set(p, ctx, kv.first, v);
    }
    fwa_buf *res = nullptr;
    exec(p, ctx, s, &res);
    peek(ctx, res, s);
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p); });
    call("fwa_buf_free", ctx, [&] { return fwa_buf_free(src); });
    call("fwa_buf_free", ctx, [&] { return fwa_buf_free(src2); });
    call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}

// two plans of one shape share tables; a destroyed plan's ring goes to the next plan; the pool is pushed over its cap; the
// context goes with pooled rings and cached tables
void cache_and_pool()
{
    const uint32_t n = 1u << 20;
    fwa_ctx *ctx = new_ctx();
    fwa_stream *s = new_stream(ctx);
    fwa_buf *a = new_src(ctx, n, 64), *b = new_src(ctx, n, 64);
    fwa_plan *p1 = new_plan(ctx, FWA_FORWARD, n, a, nullptr), *p2 = new_plan(ctx, FWA_INVERSE_SCALED, n, b, nullptr);
    check(plan_get(p1, "tables_shared") == 2 && plan_get(p2, "tables_shared") == 2, "two plans of one length do not share their tables");
    // (a create that failed behind its tables and was repeated found them in the cache: one hit more)
    check(ctx_get(ctx, "table_builds") == 1 && (R->failure_seen || ctx_get(ctx, "table_cache_hits") == 1), "the tables of one length were built twice");
    exec(p1, ctx, s);
    exec(p2, ctx, s);
    const int64_t reuses = ctx_get(ctx, "ring_reuses");
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p1); });
    fwa_plan *p3 = new_plan(ctx, FWA_FORWARD, n, a, nullptr);
    // (a tolerant run may have spent the pooled ring on the attempt that failed)
    check(R->failure_seen || ctx_get(ctx, "ring_reuses") == reuses + 1, "the ring of a destroyed plan was not taken by the next plan");
    exec(p3, ctx, nullptr);  // on another stream than p1 ran on: the ring must have drained
    // every re-tune pools the ring it replaces: 10 .. 20 transforms of 8 MiB on one chain each
    fwa_plan *p4 = new_plan(ctx, FWA_FORWARD, n, b, nullptr);
    set(p4, ctx, "streams", 1);
    int64_t pooled = 0;
    for (int64_t g = 10; g <= 20; ++g) {
        set(p4, ctx, "group", g);
        check(ctx_get(ctx, "pooled_ring_bytes") <= (1ll << 30), "the ring pool holds more than 1 GiB");
        pooled += (g - 1) << 23;  // the ring the re-tune replaced
    }
    check(pooled > (1ll << 30), "the scenario does not reach the cap of the pool");
    exec(p4, ctx, s);
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p4); });
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p2); });
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p3); });
    call("fwa_buf_free", ctx, [&] { return fwa_buf_free(a); });
    call("fwa_buf_free", ctx, [&] { return fwa_buf_free(b); });
    call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}

void buffers()
{
    fwa_ctx *c0 = new_ctx(0), *c1 = new_ctx(1);
    fwa_buf *a = new_buf(c0, 1 << 16), *b = new_buf(c0, 1 << 16), *far = new_buf(c1, 1 << 16), *view = nullptr;
    create("fwa_buf_wrap", c0, &view, [&] { return fwa_buf_wrap(c0, static_cast<char *>(fwa_buf_device_ptr(a)) + 4096, 8192, &view); });
    std::vector<char> host(1 << 16, 3);
    call("fwa_buf_upload", c0, [&] { return fwa_buf_upload(a, 0, host.data(), 1 << 16, nullptr); });
    call("fwa_buf_upload", c0, [&] { return fwa_buf_upload(b, 0, host.data(), 1 << 16, nullptr); });
    call("fwa_buf_upload", c0, [&] { return fwa_buf_upload(view, 8192 - 100, host.data() + 7, 100, nullptr); });  // the last bytes of the view
    call("fwa_buf_download", c0, [&] { return fwa_buf_download(host.data() + (1 << 16) - 128, view, 8192 - 128, 128, nullptr); });
    call("fwa_buf_copy", c0, [&] { return fwa_buf_copy(b, 1 << 15, a, 256, 1 << 15, nullptr); });
    call("fwa_buf_copy", c0, [&] { return fwa_buf_copy(b, 0, view, 0, 8192, nullptr); });
    call("fwa_ctx_synchronize", c0, [&] { return fwa_ctx_synchronize(c0); });
    // between the two devices: the explicit peer copy, on the destination's null stream and on a stream of the source's context
    int32_t kind = -1;
    call("fwa_ctx_peer_access", c0, [&] { return fwa_ctx_peer_access(c0, c1, &kind); });
    check(kind == 2, "the two simulated devices reach each other: kind must be 2");
    call("fwa_buf_copy(peer)", c1, [&] { return fwa_buf_copy(far, 0, b, 0, 1 << 16, nullptr); });
    call("fwa_ctx_synchronize", c1, [&] { return fwa_ctx_synchronize(c1); });
    fwa_stream *s0 = new_stream(c0);
    call("fwa_buf_copy(peer)", c0, [&] { return fwa_buf_copy(a, 512, far, 1024, 4096, s0); });
    call("fwa_stream_synchronize", c0, [&] { return fwa_stream_synchronize(s0); });
    // pinned staging memory
    void *pin = nullptr;
    call("fwa_host_alloc", c0, [&] { return fwa_host_alloc(c0, 4096, &pin); });
    check(pin != nullptr, "fwa_host_alloc gave no memory");
    call("fwa_buf_upload", c0, [&] { return fwa_buf_upload(a, 0, pin, 4096, s0); });
    call("fwa_buf_download_async", c0, [&] { return fwa_buf_download_async(pin, a, 4096, 4096, s0); });
    call("fwa_stream_synchronize", c0, [&] { return fwa_stream_synchronize(s0); });
    call("fwa_host_free", c0, [&] { return fwa_host_free(c0, pin); });
    // the calibration copy, both forms, and synthetic data
    call("fwa_calib_copy", c0, [&] { return fwa_calib_copy(b, a, 1 << 16, s0); });
    call("fwa_calib_copy", c0, [&] { return fwa_calib_copy(b, b, 1 << 16, s0); });
    call("fwa_fill_synthetic", c0, [&] { return fwa_fill_synthetic(view, 1, 3, 64, 0.5f, s0); });
    call("fwa_stream_synchronize", c0, [&] { return fwa_stream_synchronize(s0); });
    int64_t fr = 0, tot = 0;
    call("fwa_ctx_get_i64(mem_free_bytes)", c0, [&] { return fwa_ctx_get_i64(c0, "mem_free_bytes", &fr); });
    call("fwa_ctx_get_i64(mem_total_bytes)", c0, [&] { return fwa_ctx_get_i64(c0, "mem_total_bytes", &tot); });
    check(tot - fr == 2 << 16, "hipMemGetInfo does not answer from the books");
    call("fwa_stream_destroy", c0, [&] { return fwa_stream_destroy(s0); });
    for (fwa_buf *x : {view, a, b, far}) call("fwa_buf_free", nullptr, [&] { return fwa_buf_free(x); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(c0); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(c1); });
}

void streams_and_events()
{
    fwa_ctx *ctx = new_ctx();
    // the overlap check of the second stream rejects its first candidate (all at once takes twice as long as one alone), then
    // accepts; the third has two peers
    sim::script_elapsed_ms({0.04f, 0.04f, 0.09f, 0.09f}, 0.04f);
    fwa_stream *s1 = new_stream(ctx), *s2 = new_stream(ctx), *s3 = new_stream(ctx), *w = nullptr, *wn = nullptr;
    check(R->failure_seen || (ctx_get(ctx, "chain_rejects") == 1 && ctx_get(ctx, "chain_checks") == 3), "the overlap check did not take both outcomes");
    hipStream_t mine = raw_stream();
    create("fwa_stream_wrap", ctx, &w, [&] { return fwa_stream_wrap(ctx, mine, &w); });
    create("fwa_stream_wrap", ctx, &wn, [&] { return fwa_stream_wrap(ctx, nullptr, &wn); });
    fwa_event *e0 = nullptr, *e1 = nullptr;
    create("fwa_event_create", ctx, &e0, [&] { return fwa_event_create(ctx, &e0); });
    create("fwa_event_create", ctx, &e1, [&] { return fwa_event_create(ctx, &e1); });
    fwa_buf *buf = new_buf(ctx, 4096);
    call("fwa_event_record", ctx, [&] { return fwa_event_record(e0, s1); });
    call("fwa_fill_synthetic", ctx, [&] { return fwa_fill_synthetic(buf, 1, 0, 64, 1.0f, s1); });
    call("fwa_event_record", ctx, [&] { return fwa_event_record(e1, s1); });
    call("fwa_stream_wait_event", ctx, [&] { return fwa_stream_wait_event(s2, e1); });
    call("fwa_calib_copy", ctx, [&] { return fwa_calib_copy(buf, buf, 4096, s2); });     // behind the event: no hazard
    call("fwa_stream_wait_stream", ctx, [&] { return fwa_stream_wait_stream(w, s2); });
    call("fwa_calib_copy", ctx, [&] { return fwa_calib_copy(buf, buf, 4096, w); });      // behind the other stream
    call("fwa_stream_wait_stream", ctx, [&] { return fwa_stream_wait_stream(s3, w); });
    call("fwa_calib_copy", ctx, [&] { return fwa_calib_copy(buf, buf, 4096, s3); });
    float ms = -1;
    call("fwa_event_elapsed_ms", ctx, [&] { return fwa_event_elapsed_ms(e0, e1, &ms); });
    call("fwa_event_synchronize", ctx, [&] { return fwa_event_synchronize(e1); });
    call("fwa_stream_synchronize", ctx, [&] { return fwa_stream_synchronize(s3); });
    call("fwa_stream_synchronize", ctx, [&] { return fwa_stream_synchronize(wn); });
    // while a stream of the context captures a graph, the overlap check is refused; without the check a stream is made
    sim::set_capturing(mine, true);
    fwa_stream *s4 = nullptr;
    expect("fwa_stream_create during a capture", ctx, FWA_ERR_UNSUPPORTED, [&] {
        const int32_t st = fwa_stream_create(ctx, &s4);
        // A capture query that itself fails is read as "not capturing" (any_stream_capturing, ctx_streams.cpp) and the stream is
        // made: recorded in DESIGN.md, not asserted either way.  The scenario asks again.
        if (st == FWA_OK && sim::fired() && sim::fired_name() == "hipStreamIsCapturing" && !R->failure_seen) {
            R->failure_seen = true;
            (void)fwa_stream_destroy(s4);
            return fwa_stream_create(ctx, &s4);
        }
        return st;
    });
    check(s4 == nullptr, "a refused fwa_stream_create left *out set");
    call("fwa_ctx_set_i64", ctx, [&] { return fwa_ctx_set_i64(ctx, "chain_check", 0); });
    s4 = new_stream(ctx);
    sim::set_capturing(mine, false);
    // the context goes first: every handle then answers INVALID_ARG and can still be destroyed
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
    expect("fwa_stream_synchronize after its context", nullptr, FWA_ERR_INVALID_ARG, [&] { return fwa_stream_synchronize(s1); });
    expect("fwa_event_record after its context", nullptr, FWA_ERR_INVALID_ARG, [&] { return fwa_event_record(e0, s1); });
    expect("fwa_event_synchronize after its context", nullptr, FWA_ERR_INVALID_ARG, [&] { return fwa_event_synchronize(e1); });
    char c[8];
    expect("fwa_buf_download after its context", nullptr, FWA_ERR_INVALID_ARG, [&] { return fwa_buf_download(c, buf, 0, 8, nullptr); });
    expect("fwa_stream_wait_stream after its context", nullptr, FWA_ERR_INVALID_ARG, [&] { return fwa_stream_wait_stream(s2, s3); });
    for (fwa_stream *s : {s1, s2, s3, s4, w, wn}) call("fwa_stream_destroy", nullptr, [&] { return fwa_stream_destroy(s); });
    for (fwa_event *e : {e0, e1}) call("fwa_event_destroy", nullptr, [&] { return fwa_event_destroy(e); });
    call("fwa_buf_free", nullptr, [&] { return fwa_buf_free(buf); });
    raw_stream_destroy(mine);
}

// A plan destroyed right after an exec on a stream the library made, on a wrapped one, and on one already destroyed: the three
// branches of the marker logic in fwa_plan_destroy.  Each time the next plan of the shape takes the pooled ring and runs on
// ANOTHER stream at once: if the destroy had not waited, that is a hazard on the ring.
void destroy_in_flight(int branch)
{
    const uint32_t n = 1u << 16;
    fwa_ctx *ctx = new_ctx();
    fwa_stream *owned = new_stream(ctx), *other = new_stream(ctx), *wrapped = nullptr;
    hipStream_t mine = raw_stream();
    create("fwa_stream_wrap", ctx, &wrapped, [&] { return fwa_stream_wrap(ctx, mine, &wrapped); });
    fwa_buf *a = new_src(ctx, n, 9), *b = new_src(ctx, n, 9);
    fwa_plan *p = new_plan(ctx, FWA_FORWARD, n, a, nullptr);
    exec(p, ctx, branch == 1 || branch == 3 ? wrapped : owned);
    if (branch == 2) { call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(owned); }); owned = nullptr; }
    // branch 3: another stream of the device captures a graph, so the device-wide wait behind a wrapped stream is illegal and
    // fails: the ring may still be in use and must not reach the pool
    if (branch == 3) sim::set_capturing(owned->s, true);
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p); });
    if (branch == 3) {
        check(ctx_get(ctx, "pooled_ring_bytes") == 0, "a plan destroyed while its last exec could not be waited for pooled its ring");
        sim::set_capturing(owned->s, false);
    }
    fwa_plan *q = new_plan(ctx, FWA_INVERSE_SCALED, n, b, nullptr);
    exec(q, ctx, other);
    call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(q); });
    call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
    for (fwa_buf *x : {a, b}) call("fwa_buf_free", ctx, [&] { return fwa_buf_free(x); });
    for (fwa_stream *s : {owned, other, wrapped}) call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    raw_stream_destroy(mine);
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}

// the side libraries: create, exec twice, destroy
template <class Plan>
void side_run(fwa_ctx *ctx, fwa_stream *s, const char *what, Plan *p, int32_t (*get)(const Plan *, const char *, int64_t *),
              int32_t (*run)(Plan *, fwa_stream *), int32_t (*destroy)(Plan *))
{
    int64_t launches = -1;
    check(get(p, "launches_per_exec", &launches) == FWA_OK, "launches_per_exec");
    for (int i = 0; i < 2; ++i) exec_checked(what, ctx, s, launches, [&] { return run(p, s); });
    call("destroy of a side-library plan", ctx, [&] { return destroy(p); });
}
void side_libraries(bool large)
{
    fwa_ctx *ctx = new_ctx();
    fwa_stream *s = new_stream(ctx);
    {   // strided: the columns of batch matrices of n rows x howmany columns
        const uint32_t n = large ? 4096 : 64;
        const uint64_t howmany = large ? 40 : 48, batch = large ? 2 : 3;
        fwa_buf *buf = new_src(ctx, n * howmany, batch);
        fws_plan *p = nullptr;
        create("fws_plan_create", ctx, &p, [&] { return fws_plan_create(ctx, FWA_FORWARD, n, howmany, buf, &p); });
        side_run<fws_plan>(ctx, s, "fws_plan_exec", p, fws_plan_get_i64, fws_plan_exec, fws_plan_destroy);
        call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
        call("fwa_buf_free", ctx, [&] { return fwa_buf_free(buf); });
    }
    {   // 2-D: fused (one launch) and rows + columns (two launches: the plan holds a strided plan inside)
        const uint32_t rows = large ? 256 : 16, cols = large ? 128 : 16;
        fwa_buf *buf = new_src(ctx, (uint64_t)rows * cols, large ? 2 : 5);
        fw2_plan *p = nullptr;
        create("fw2_plan_create", ctx, &p, [&] { return fw2_plan_create(ctx, FWA_INVERSE_SCALED, rows, cols, buf, &p); });
        int64_t l = 0;
        check(fw2_plan_get_i64(p, "launches_per_exec", &l) == FWA_OK && l == (large ? 2 : 1), "2-D launches_per_exec");
        side_run<fw2_plan>(ctx, s, "fw2_plan_exec", p, fw2_plan_get_i64, fw2_plan_exec, fw2_plan_destroy);
        call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
        call("fwa_buf_free", ctx, [&] { return fwa_buf_free(buf); });
    }
    {   // real: forward (small), inverse (large)
        const uint32_t n = large ? 4096 : 64;
        const uint64_t batch = large ? 3 : 7;
        fwa_buf *re = new_buf(ctx, 4ull * n * batch), *sp = new_buf(ctx, 8ull * (n / 2 + 1) * batch);
        fill(ctx, large ? sp : re, n);
        fwr_plan *p = nullptr;
        create("fwr_plan_create", ctx, &p, [&] { return fwr_plan_create(ctx, large ? FWA_INVERSE_UNSCALED : FWA_FORWARD, n, large ? sp : re, large ? re : sp, &p); });
        side_run<fwr_plan>(ctx, s, "fwr_plan_exec", p, fwr_plan_get_i64, fwr_plan_exec, fwr_plan_destroy);
        call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
        for (fwa_buf *x : {re, sp}) call("fwa_buf_free", ctx, [&] { return fwa_buf_free(x); });
    }
    {   // convolution: out of place with two filters (small), in place with one (large)
        const uint32_t n = large ? 4096 : 128;
        const uint64_t batch = large ? 4 : 6, filters = large ? 1 : 2;
        fwa_buf *src = new_src(ctx, n, batch), *flt = new_src(ctx, n, filters), *dst = large ? src : new_buf(ctx, 8ull * n * batch);
        fwc_plan *p = nullptr;
        create("fwc_plan_create", ctx, &p, [&] { return fwc_plan_create(ctx, FWA_INVERSE_SCALED, large ? FWC_CONJ_FILTER : 0u, n, src, flt, dst, &p); });
        side_run<fwc_plan>(ctx, s, "fwc_plan_exec", p, fwc_plan_get_i64, fwc_plan_exec, fwc_plan_destroy);
        call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
        for (fwa_buf *x : {src, flt}) call("fwa_buf_free", ctx, [&] { return fwa_buf_free(x); });
        if (dst != src) call("fwa_buf_free", ctx, [&] { return fwa_buf_free(dst); });
    }
    call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}

// ================================================ communicators ================================================
// A collective or a sendrecv of one rank.  Whatever it answers, its group must be closed when it returns.  A failure by injection is
// checked by failed() and ends the collective: the header calls it fatal for the communicator, the scenario destroys everything.
template <class F>
void comm_call(const char *what, const fwa_ctx *ctx, F f)
{
    const int32_t st = f();
    (void)sim::rccl_group_closed(what);
    if (failed(st, what, ctx)) { R->gave_up = true; throw GiveUp(); }
}
// A call the header says is refused with FWA_ERR_INVALID_ARG: it has posted and enqueued nothing.
template <class F>
void comm_refused(const std::string &what, const fwa_ctx *ctx, F f)
{
    const uint64_t pending = sim::rccl_pending(), calls = sim::injectable_calls();
    const size_t records = sim::rccl_records().size(), ops = sim::ops().size();
    expect(what.c_str(), ctx, FWA_ERR_INVALID_ARG, f);
    (void)sim::rccl_group_closed(what);
    check(sim::rccl_pending() == pending && sim::rccl_records().size() == records && sim::ops().size() == ops && sim::injectable_calls() == calls,
          what + " was refused and still reached the runtime or RCCL");
}

struct Rank { fwa_ctx *ctx = nullptr; fwa_stream *s = nullptr; fwa_comm *c = nullptr; };
struct World {
    int world = 0;
    std::vector<Rank> r;
    std::vector<fwa_buf *> bufs;    // what the scenario holds, so that a collective given up half-way leaves nothing behind
    std::vector<fwa_plan *> plans;
};
// Every comm scenario begins here: the id comes from the simulated RCCL, whose call counter must move -- with an installed RCCL in
// its place a real HIP runtime would be in the process.
void unique_id(uint8_t id[FWA_COMM_ID_BYTES])
{
    const uint64_t before = sim::rccl_calls();
    call("fwa_comm_unique_id", nullptr, [&] { return fwa_comm_unique_id(id); });
    if (sim::rccl_calls() == before) {
        check(false, "the call counter of the simulated RCCL did not move: another librccl.so.1 answered");
        throw Abort();
    }
}
void make_world(World &w, int world, int first_device = 0)
{
    uint8_t id[FWA_COMM_ID_BYTES];
    unique_id(id);
    w.world = world;
    w.r.resize((size_t)world);
    for (int r = 0; r < world; ++r) {  // a context on a device of its own, a stream of its own
        Rank &k = w.r[(size_t)r];
        k.ctx = new_ctx(first_device + r);
        k.s = new_stream(k.ctx);
        create("fwa_comm_create", k.ctx, &k.c, [&] { return fwa_comm_create(k.ctx, id, world, r, &k.c); });
    }
}
fwa_buf *add_buf(World &w, fwa_ctx *ctx, uint64_t bytes)
{
    w.bufs.push_back(nullptr);  // (no allocation between the create and the note of it)
    fwa_buf *b = new_buf(ctx, bytes);
    w.bufs.back() = b;
    return b;
}
void release(World &w)  // plans and buffers
{
    for (const Rank &k : w.r)
        if (k.ctx) call("fwa_ctx_synchronize", k.ctx, [&] { return fwa_ctx_synchronize(k.ctx); });
    for (fwa_plan *p : w.plans) call("fwa_plan_destroy", nullptr, [&] { return fwa_plan_destroy(p); });
    w.plans.clear();
    for (auto it = w.bufs.rbegin(); it != w.bufs.rend(); ++it) call("fwa_buf_free", nullptr, [&] { return fwa_buf_free(*it); });  // views first
    w.bufs.clear();
}
void destroy_world(World &w)
{
    release(w);
    for (Rank &k : w.r) call("fwa_comm_destroy", k.ctx, [&] { return fwa_comm_destroy(k.c); });  // drops what its rank left pending
    check(sim::rccl_pending() == 0 && sim::rccl_live() == 0, "operations or communicators are left after the last fwa_comm_destroy");
    for (Rank &k : w.r) call("fwa_stream_destroy", k.ctx, [&] { return fwa_stream_destroy(k.s); });
    for (Rank &k : w.r) call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(k.ctx); });
    w.r.clear();
}

uint64_t dev_ptr(const fwa_buf *b, uint64_t off = 0) { return reinterpret_cast<uint64_t>(fwa_buf_device_ptr(b)) + off; }
using Moved = std::tuple<int, uint64_t, uint64_t, int, uint64_t>;  // source rank, address, bytes, destination rank, address
void records_are(std::vector<Moved> want, const std::string &what)
{
    std::vector<Moved> got;
    for (const sim::RcclRecord &r : sim::rccl_records()) got.emplace_back(r.src_rank, r.src, r.bytes, r.dst_rank, r.dst);
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    if (got == want) return;
    std::string d = what + ": the transfer records differ from the slab rule: " + std::to_string(got.size()) + " recorded, " + std::to_string(want.size()) + " expected";
    for (size_t i = 0; i < got.size() || i < want.size(); ++i)
        if (i >= got.size() || i >= want.size() || got[i] != want[i]) {
            char t[200];
            const Moved *m = i < got.size() ? &got[i] : &want[i];
            std::snprintf(t, sizeof t, "; first difference (%s): rank %d %#llx +%llu -> rank %d %#llx", i < got.size() ? "recorded" : "missing", std::get<0>(*m),
                          (unsigned long long)std::get<1>(*m), (unsigned long long)std::get<2>(*m), std::get<3>(*m), (unsigned long long)std::get<4>(*m));
            d += t;
            break;
        }
    check(false, d);
}
// the device copies among ops()[first ..]: `want` of them (0 or 1), and that one from src to dst; everything else there is a transfer
void copies_are(size_t first, uint64_t want, uint64_t src, uint64_t dst, uint64_t bytes, const std::string &what)
{
    uint64_t copies = 0, others = 0;
    for (size_t i = first; i < sim::ops().size(); ++i) {
        const sim::Op &o = sim::ops()[i];
        if (o.name == "hipMemcpyAsync") {
            ++copies;
            check(o.reads.size() == 1 && o.reads[0].lo == src && o.reads[0].hi == src + bytes && o.writes.size() == 1 && o.writes[0].lo == dst && o.writes[0].hi == dst + bytes,
                  what + ": the device copy of the root's own slab moves other bytes than the slab rule says");
        } else if (o.name.compare(0, 8, "transfer") != 0) ++others;
    }
    check(copies == want && others == 0, what + ": " + std::to_string(copies) + " device copies and " + std::to_string(others) + " other operations, expected " +
                                             std::to_string(want) + " and 0");
}
// every byte of [lo, hi) written exactly once by ops()[first ..], but for [hole_lo, hole_hi), which stays in place
void written_once(size_t first, uint64_t lo, uint64_t hi, uint64_t hole_lo, uint64_t hole_hi, const std::string &what)
{
    std::vector<sim::Range> w;
    for (size_t i = first; i < sim::ops().size(); ++i)
        for (const sim::Range &r : sim::ops()[i].writes)
            if (r.lo < hi && lo < r.hi) w.push_back(r);
    if (hole_lo < hole_hi) w.push_back({hole_lo, hole_hi});
    std::sort(w.begin(), w.end(), [](const sim::Range &a, const sim::Range &b) { return a.lo < b.lo; });
    uint64_t at = lo;
    for (const sim::Range &r : w) {
        if (r.lo != at) {
            char t[160];
            std::snprintf(t, sizeof t, ": byte %llu of the destination is written %s", (unsigned long long)((r.lo < at ? r.lo : at) - lo), r.lo < at ? "twice" : "never");
            check(false, what + t);
            return;
        }
        at = r.hi;
    }
    check(at == hi, what + ": the end of the destination is never written");
}
std::vector<int> rank_order(int world, int root, int order)  // 0: root first, 1: root last, 2: root in the middle of the others
{
    std::vector<int> others, v;
    for (int r = 0; r < world; ++r)
        if (r != root) others.push_back(r);
    const size_t before = order == 0 ? 0 : order == 1 ? others.size() : others.size() / 2;
    v.assign(others.begin(), others.begin() + (std::ptrdiff_t)before);
    v.push_back(root);
    v.insert(v.end(), others.begin() + (std::ptrdiff_t)before, others.end());
    return v;
}

// One case: scatter, one forward exec per rank on its slab, gather, on every rank in the given order.  `alias`: the root's slab IS its
// part of the batch (a view), so that the scatter copies nothing.
void slab_case(World &w, uint32_t n, uint64_t batch, int root, int order, bool alias)
{
    const int W = w.world;
    const uint64_t tb = 8ull * n;
    const std::string tag = "world " + std::to_string(W) + " root " + std::to_string(root) + " n " + std::to_string(n) + " batch " + std::to_string(batch) + " order " +
                            std::to_string(order) + (alias ? " alias" : "");
    // the slab rule, restated: batch = q W + e; the first e ranks own q + 1 transforms, the others q, in rank order
    std::vector<uint64_t> first((size_t)W), count((size_t)W);
    const uint64_t q = batch / (uint64_t)W, e = batch % (uint64_t)W;
    for (int r = 0; r < W; ++r) {
        count[(size_t)r] = q + ((uint64_t)r < e ? 1 : 0);
        first[(size_t)r] = r == 0 ? 0 : first[(size_t)r - 1] + count[(size_t)r - 1];
    }
    const Rank &top = w.r[(size_t)root];
    const uint64_t own_first = first[(size_t)root] * tb, own_bytes = count[(size_t)root] * tb;
    alias = alias && own_bytes;
    fwa_buf *full = add_buf(w, top.ctx, batch * tb), *result = alias ? full : add_buf(w, top.ctx, batch * tb);
    if (batch) fill(top.ctx, full, n);
    std::vector<fwa_buf *> slab((size_t)W), out((size_t)W);
    for (int r = 0; r < W; ++r) {
        fwa_buf *&b = slab[(size_t)r];
        if (r == root && alias) {
            w.bufs.push_back(nullptr);
            create("fwa_buf_wrap", top.ctx, &b, [&] { return fwa_buf_wrap(top.ctx, static_cast<char *>(fwa_buf_device_ptr(full)) + own_first, own_bytes, &b); });
            w.bufs.back() = b;
        } else b = add_buf(w, w.r[(size_t)r].ctx, count[(size_t)r] * tb);  // exactly its count: an empty slab is a buffer of no bytes
    }
    const std::vector<int> ranks = rank_order(W, root, order);

    sim::rccl_clear_records();
    size_t op0 = sim::ops().size();
    for (int r : ranks) {
        const Rank &k = w.r[(size_t)r];
        comm_call("fwa_comm_scatter", k.ctx, [&] { return fwa_comm_scatter(k.c, root, r == root ? full : nullptr, slab[(size_t)r], n, batch, k.s); });
    }
    (void)sim::rccl_complete(tag + ", scatter");
    std::vector<Moved> want;
    for (int p = 0; p < W; ++p)
        if (p != root && count[(size_t)p]) want.emplace_back(root, dev_ptr(full, first[(size_t)p] * tb), count[(size_t)p] * tb, p, dev_ptr(slab[(size_t)p]));
    records_are(want, tag + ", scatter");
    copies_are(op0, own_bytes && !alias ? 1 : 0, dev_ptr(full, own_first), dev_ptr(slab[(size_t)root]), own_bytes, tag + ", scatter");

    for (int r : ranks) {
        out[(size_t)r] = slab[(size_t)r];
        if (!count[(size_t)r]) continue;
        const Rank &k = w.r[(size_t)r];
        w.plans.push_back(nullptr);
        fwa_plan *p = new_plan(k.ctx, FWA_FORWARD, n, slab[(size_t)r], nullptr);
        w.plans.back() = p;
        exec(p, k.ctx, k.s, &out[(size_t)r]);
    }

    sim::rccl_clear_records();
    op0 = sim::ops().size();
    for (int r : ranks) {
        const Rank &k = w.r[(size_t)r];
        comm_call("fwa_comm_gather", k.ctx, [&] { return fwa_comm_gather(k.c, root, out[(size_t)r], r == root ? result : nullptr, n, batch, k.s); });
    }
    (void)sim::rccl_complete(tag + ", gather");
    want.clear();
    for (int p = 0; p < W; ++p)
        if (p != root && count[(size_t)p]) want.emplace_back(p, dev_ptr(out[(size_t)p]), count[(size_t)p] * tb, root, dev_ptr(result, first[(size_t)p] * tb));
    records_are(want, tag + ", gather");
    const bool in_place = own_bytes && dev_ptr(out[(size_t)root]) == dev_ptr(result, own_first);  // the exec left the result in the view
    copies_are(op0, own_bytes && !in_place ? 1 : 0, dev_ptr(out[(size_t)root]), dev_ptr(result, own_first), own_bytes, tag + ", gather");
    written_once(op0, dev_ptr(result), dev_ptr(result) + batch * tb, in_place ? dev_ptr(result, own_first) : 0, in_place ? dev_ptr(result, own_first) + own_bytes : 0,
                 tag + ", gather");
    release(w);
}

// The clean audit of one world size: every root, n = 2, 512 and 2^20, batches 0, 1, W - 1, W, 3 W + 2, the three orders; and one batch whose
// full buffer on the root passes 4 GiB.
void comm_audit(int world)
{
    World w;
    try {
        make_world(w, world);
        for (uint32_t n : {2u, 512u, 1u << 20}) {
            const std::set<uint64_t> batches = {0, 1, (uint64_t)world - 1, (uint64_t)world, 3 * (uint64_t)world + 2};
            for (int root = 0; root < world; ++root)
                for (uint64_t batch : batches)
                    for (int order = 0; order < 3; ++order) slab_case(w, n, batch, root, order, (root + order + (int)batch) % 3 == 2);
        }
        slab_case(w, 1u << 20, 513 + (uint64_t)world, world - 1, world % 3, false);  // 8 MiB a transform: 4 GiB and a little
    } catch (const GiveUp &) {
    }
    destroy_world(w);
}
void comm_small(int world, uint32_t n, uint64_t batch, int root, int order, bool alias)
{
    World w;
    try {
        make_world(w, world);
        slab_case(w, n, batch, root, order, alias);
    } catch (const GiveUp &) {
    }
    destroy_world(w);
}

// fwa_comm_sendrecv: a ring shift, every rank sending another byte count from another offset, the receive ending at the end of its buffer
void comm_ring(int world)
{
    World w;
    try {
        make_world(w, world);
        const uint64_t size = 8192;
        std::vector<fwa_buf *> snd((size_t)world), rcv((size_t)world);
        auto bytes = [](int r) { return 1024ull + 8 * (uint64_t)r; };
        for (int r = 0; r < world; ++r) {
            snd[(size_t)r] = add_buf(w, w.r[(size_t)r].ctx, size);
            rcv[(size_t)r] = add_buf(w, w.r[(size_t)r].ctx, size);
            fill(w.r[(size_t)r].ctx, snd[(size_t)r], 4);
        }
        sim::rccl_clear_records();
        std::vector<Moved> want;
        std::vector<int> drive;  // the odd ranks, then the even ones
        for (int r = 1; r < world; r += 2) drive.push_back(r);
        for (int r = 0; r < world; r += 2) drive.push_back(r);
        for (int r : drive) {
            const int to = (r + 1) % world, from = (r + world - 1) % world;
            const Rank &k = w.r[(size_t)r];
            comm_call("fwa_comm_sendrecv", k.ctx, [&] {
                return fwa_comm_sendrecv(k.c, snd[(size_t)r], 16 * (uint64_t)r, bytes(r), to, rcv[(size_t)r], size - bytes(from), bytes(from), from, k.s);
            });
            want.emplace_back(r, dev_ptr(snd[(size_t)r], 16 * (uint64_t)r), bytes(r), to, dev_ptr(rcv[(size_t)to], size - bytes(r)));
        }
        (void)sim::rccl_complete("ring shift over " + std::to_string(world) + " ranks");
        records_are(want, "ring shift over " + std::to_string(world) + " ranks");
        for (int r = 0; r < world; ++r) {  // what arrived can be read, on the stream it arrived on
            char host[64];
            const Rank &k = w.r[(size_t)r];
            call("fwa_buf_download", k.ctx, [&] { return fwa_buf_download(host, rcv[(size_t)r], size - 64, 64, k.s); });
        }
    } catch (const GiveUp &) {
    }
    destroy_world(w);
}

// the forms of fwa_comm_sendrecv, and what it refuses
void comm_forms()
{
    World w;
    try {
        make_world(w, 2);
        const Rank &r0 = w.r[0], &r1 = w.r[1];
        fwa_buf *a0 = add_buf(w, r0.ctx, 8192), *b0 = add_buf(w, r0.ctx, 8192), *b1 = add_buf(w, r1.ctx, 8192);
        fill(r0.ctx, a0, 4);
        sim::rccl_clear_records();
        // a send alone, and a receive alone
        comm_call("fwa_comm_sendrecv(send only)", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 8, 512, 1, nullptr, 0, 0, -1, r0.s); });
        check(sim::rccl_pending() == 1, "a send whose receive is not posted yet must wait");
        comm_call("fwa_comm_sendrecv(receive only)", r1.ctx, [&] { return fwa_comm_sendrecv(r1.c, nullptr, 0, 0, -1, b1, 16, 512, 0, r1.s); });
        // to the rank itself, with its receive: a local copy
        comm_call("fwa_comm_sendrecv(self)", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 0, 256, 0, b0, 1024, 256, 0, r0.s); });
        // neither side: an empty group
        comm_call("fwa_comm_sendrecv(nothing)", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, nullptr, 0, 0, -1, nullptr, 0, 0, -1, r0.s); });
        (void)sim::rccl_complete("the forms of sendrecv");
        records_are({Moved(0, dev_ptr(a0, 8), 512, 1, dev_ptr(b1, 16)), Moved(0, dev_ptr(a0), 256, 0, dev_ptr(b0, 1024))}, "the forms of sendrecv");
        // refused, with nothing posted
        comm_refused("a send to the rank itself without its receive", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 0, 256, 0, nullptr, 0, 0, -1, r0.s); });
        comm_refused("a receive from the rank itself without its send", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, nullptr, 0, 0, -1, b0, 0, 256, 0, r0.s); });
        comm_refused("a send to the rank itself and a receive from the peer", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 0, 256, 0, b0, 0, 256, 1, r0.s); });
        comm_refused("unequal sizes to the rank itself", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 0, 256, 0, b0, 0, 128, 0, r0.s); });
        comm_refused("send_to = world", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 0, 256, 2, nullptr, 0, 0, -1, r0.s); });
        comm_refused("recv_from = world", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, nullptr, 0, 0, -1, b0, 0, 256, 2, r0.s); });
        comm_refused("a send range one byte past the buffer", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 8192 - 100, 101, 1, nullptr, 0, 0, -1, r0.s); });
        comm_refused("a send offset past the buffer", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 8193, 0, 1, nullptr, 0, 0, -1, r0.s); });
        comm_refused("a send size that wraps with its offset", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 16, ~0ull - 7, 1, nullptr, 0, 0, -1, r0.s); });
        comm_refused("a receive range one byte past the buffer", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, nullptr, 0, 0, -1, b0, 8192 - 100, 101, 1, r0.s); });
        comm_refused("a send without a buffer", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, nullptr, 0, 0, 1, nullptr, 0, 0, -1, r0.s); });
        comm_refused("a stream of the peer's context", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, a0, 0, 256, 1, nullptr, 0, 0, -1, r1.s); });
        comm_refused("a scatter on a stream of the peer's context", r0.ctx, [&] { return fwa_comm_scatter(r0.c, 0, a0, b0, 4, 8, r1.s); });
        comm_refused("a root outside the world", r0.ctx, [&] { return fwa_comm_gather(r0.c, 2, b0, a0, 4, 8, r0.s); });
        comm_refused("a root without the full buffer", r0.ctx, [&] { return fwa_comm_scatter(r0.c, 0, nullptr, b0, 4, 8, r0.s); });
        comm_refused("a full buffer one transform short", r0.ctx, [&] { return fwa_comm_scatter(r0.c, 0, a0, b0, 4, 257, r0.s); });
    } catch (const GiveUp &) {
    }
    destroy_world(w);
}

// Buffers and streams of another context or of a destroyed one in every position, and a communicator that outlives its context: what
// the header says the caller gets, with the sanitizer silent.
void comm_lifetimes()
{
    World w;
    fwa_buf *gone_buf = nullptr, *late_buf = nullptr;
    fwa_stream *gone_stream = nullptr, *late_stream = nullptr;
    fwa_comm *late = nullptr;
    try {
        make_world(w, 2);
        const Rank &r0 = w.r[0], &r1 = w.r[1];
        const uint32_t n = 4;
        const uint64_t batch = 8, tb = 8ull * n;
        fwa_buf *full = add_buf(w, r0.ctx, batch * tb), *slab = add_buf(w, r0.ctx, batch * tb), *foreign = add_buf(w, r1.ctx, batch * tb);
        fill(r0.ctx, full, n);
        fill(r1.ctx, foreign, n);
        fwa_ctx *gone = new_ctx(2);
        gone_stream = new_stream(gone);
        gone_buf = new_buf(gone, batch * tb);
        call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(gone); });
        for (fwa_buf *bad : {foreign, gone_buf}) {
            const std::string whose = bad == foreign ? " of another context" : " of a destroyed context";
            comm_refused("a send buffer" + whose, r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, bad, 0, 64, 1, nullptr, 0, 0, -1, r0.s); });
            comm_refused("a receive buffer" + whose, r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, nullptr, 0, 0, -1, bad, 0, 64, 1, r0.s); });
            comm_refused("a self send from a buffer" + whose, r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, bad, 0, 64, 0, slab, 0, 64, 0, r0.s); });
            comm_refused("a slab buffer" + whose + " (root, scatter)", r0.ctx, [&] { return fwa_comm_scatter(r0.c, 0, full, bad, n, batch, r0.s); });
            comm_refused("a slab buffer" + whose + " (not root, gather)", r0.ctx, [&] { return fwa_comm_gather(r0.c, 1, bad, nullptr, n, batch, r0.s); });
            comm_refused("a full buffer" + whose + " (scatter)", r0.ctx, [&] { return fwa_comm_scatter(r0.c, 0, bad, slab, n, batch, r0.s); });
            comm_refused("a full buffer" + whose + " (gather)", r0.ctx, [&] { return fwa_comm_gather(r0.c, 0, slab, bad, n, batch, r0.s); });
        }
        comm_refused("a stream of a destroyed context (sendrecv)", r0.ctx, [&] { return fwa_comm_sendrecv(r0.c, full, 0, 64, 1, nullptr, 0, 0, -1, gone_stream); });
        comm_refused("a stream of a destroyed context (scatter)", r0.ctx, [&] { return fwa_comm_scatter(r0.c, 0, full, slab, n, batch, gone_stream); });
        // a communicator whose context goes first: a world of its own, one rank, on a fourth device
        uint8_t id[FWA_COMM_ID_BYTES];
        unique_id(id);
        fwa_ctx *early = new_ctx(3);
        late_stream = new_stream(early);
        late_buf = new_buf(early, batch * tb);
        create("fwa_comm_create", early, &late, [&] { return fwa_comm_create(early, id, 1, 0, &late); });
        call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(early); });
        int64_t v = -1;
        call("fwa_comm_get_i64(rank) after its context", nullptr, [&] { return fwa_comm_get_i64(late, "rank", &v); });
        check(v == 0, "rank of a communicator after its context");
        call("fwa_comm_get_i64(world) after its context", nullptr, [&] { return fwa_comm_get_i64(late, "world", &v); });
        check(v == 1, "world of a communicator after its context");
        call("fwa_comm_get_i64(device) after its context", nullptr, [&] { return fwa_comm_get_i64(late, "device", &v); });
        check(v == 3, "device of a communicator after its context");
        comm_refused("an unknown key after its context", nullptr, [&] { return fwa_comm_get_i64(late, "nothing", &v); });
        comm_refused("a scatter after the communicator's context", nullptr, [&] { return fwa_comm_scatter(late, 0, late_buf, late_buf, n, batch, nullptr); });
        comm_refused("a gather after the communicator's context", nullptr, [&] { return fwa_comm_gather(late, 0, late_buf, late_buf, n, batch, late_stream); });
        comm_refused("a sendrecv after the communicator's context", nullptr, [&] { return fwa_comm_sendrecv(late, late_buf, 0, 64, 0, late_buf, 64, 64, 0, nullptr); });
    } catch (const GiveUp &) {
    }
    call("fwa_comm_destroy after its context", nullptr, [&] { return fwa_comm_destroy(late); });
    for (fwa_buf *b : {gone_buf, late_buf}) call("fwa_buf_free", nullptr, [&] { return fwa_buf_free(b); });
    for (fwa_stream *s : {gone_stream, late_stream}) call("fwa_stream_destroy", nullptr, [&] { return fwa_stream_destroy(s); });
    destroy_world(w);
}

// The hazard the header documents, as a positive test of the fake: one rank's arguments are rejected, it posts nothing, and what its
// peers have posted for it waits for ever.
void comm_documented_hazard()
{
    World w;
    try {
        make_world(w, 3);
        const uint32_t n = 8;
        const uint64_t batch = 7, tb = 8ull * n;  // slabs of 3, 2, 2
        fwa_buf *full = add_buf(w, w.r[0].ctx, batch * tb);
        fill(w.r[0].ctx, full, n);
        fwa_buf *s0 = add_buf(w, w.r[0].ctx, 3 * tb), *s1 = add_buf(w, w.r[1].ctx, 1 * tb) /* one transform short */, *s2 = add_buf(w, w.r[2].ctx, 2 * tb);
        comm_call("fwa_comm_scatter", w.r[0].ctx, [&] { return fwa_comm_scatter(w.r[0].c, 0, full, s0, n, batch, w.r[0].s); });
        comm_refused("a slab buffer one transform short", w.r[1].ctx, [&] { return fwa_comm_scatter(w.r[1].c, 0, nullptr, s1, n, batch, w.r[1].s); });
        comm_call("fwa_comm_scatter", w.r[2].ctx, [&] { return fwa_comm_scatter(w.r[2].c, 0, nullptr, s2, n, batch, w.r[2].s); });
        const uint64_t left = sim::rccl_complete("scatter with rank 1 rejected");
        check(left == 1, "the root's send to the rejected rank must be the one operation left, " + std::to_string(left) + " are");
        sim::expect_violations(sim::V_UNMATCHED, 1, "the documented hazard");
    } catch (const GiveUp &) {
    }
    destroy_world(w);
}

// scatter, exec, gather over three ranks driven through fft_wgpu::Comm (include/fft_wgpu.hpp): the mirror throws where the C ABI answers
// a status, and its destructors are the teardown
void comm_mirror()
{
    namespace fw = fft_wgpu;
    const int W = 3, root = 1;
    const uint32_t n = 512;
    const uint64_t batch = 3 * W + 2, tb = 8ull * n;
    try {
        const uint64_t before = sim::rccl_calls();
        const fw::Comm::Id id = fw::Comm::unique_id();
        if (sim::rccl_calls() == before) { check(false, "the call counter of the simulated RCCL did not move: another librccl.so.1 answered"); throw Abort(); }
        std::vector<std::unique_ptr<fw::Device>> dev;
        std::vector<std::unique_ptr<fw::CommandEncoder>> enc;
        std::vector<std::unique_ptr<fw::Buffer>> slab;
        std::vector<std::unique_ptr<fw::Comm>> comm;
        std::vector<std::unique_ptr<fw::Forward>> plan;
        for (int r = 0; r < W; ++r) {
            dev.emplace_back(new fw::Device(r));
            enc.emplace_back(new fw::CommandEncoder(*dev.back()));
        }
        fw::Buffer full(*dev[(size_t)root], batch * tb), result(*dev[(size_t)root], batch * tb);
        std::vector<uint64_t> first, count;
        for (int r = 0; r < W; ++r) {
            comm.emplace_back(new fw::Comm(*dev[(size_t)r], id, W, r));
            count.push_back(batch / W + ((uint64_t)r < batch % W ? 1 : 0));
            first.push_back(r ? first.back() + count[(size_t)r - 1] : 0);
            const fw::Slab mine = comm.back()->my_slab(batch);
            check(mine.first == first.back() && mine.count == count.back(), "fft_wgpu::Comm::my_slab differs from the slab rule");
            slab.emplace_back(new fw::Buffer(*dev[(size_t)r], count.back() * tb));
        }
        std::vector<char> host(batch * tb, 1);
        full.write(host.data(), host.size(), enc[(size_t)root].get());  // on the stream the scatter follows on
        sim::rccl_clear_records();
        for (int r : rank_order(W, root, 2)) comm[(size_t)r]->scatter(root, r == root ? &full : nullptr, *slab[(size_t)r], n, batch, *enc[(size_t)r]);
        (void)sim::rccl_group_closed("fft_wgpu::Comm::scatter");
        (void)sim::rccl_complete("mirror, scatter");
        std::vector<Moved> want;
        for (int p = 0; p < W; ++p)
            if (p != root) want.emplace_back(root, dev_ptr(full.raw(), first[(size_t)p] * tb), count[(size_t)p] * tb, p, dev_ptr(slab[(size_t)p]->raw()));
        records_are(want, "mirror, scatter");
        std::vector<fw::Buffer *> out;
        for (int r = 0; r < W; ++r) {
            plan.emplace_back(new fw::Forward(*dev[(size_t)r], *dev[(size_t)r], *slab[(size_t)r], n));
            out.push_back(&plan.back()->proc(*enc[(size_t)r]));
        }
        sim::rccl_clear_records();
        const size_t op0 = sim::ops().size();
        for (int r : rank_order(W, root, 1)) comm[(size_t)r]->gather(root, *out[(size_t)r], r == root ? &result : nullptr, n, batch, *enc[(size_t)r]);
        (void)sim::rccl_group_closed("fft_wgpu::Comm::gather");
        (void)sim::rccl_complete("mirror, gather");
        want.clear();
        for (int p = 0; p < W; ++p)
            if (p != root) want.emplace_back(p, dev_ptr(out[(size_t)p]->raw()), count[(size_t)p] * tb, root, dev_ptr(result.raw(), first[(size_t)p] * tb));
        records_are(want, "mirror, gather");
        written_once(op0, dev_ptr(result.raw()), dev_ptr(result.raw()) + batch * tb, 0, 0, "mirror, gather");
        for (int r = 0; r < W; ++r) enc[(size_t)r]->synchronize();
    } catch (const fw::Error &e) {
        (void)sim::rccl_group_closed("a call of the mirror that threw");
        if (!R->tolerant || !sim::fired() || R->failure_seen) { check(false, std::string("the mirror threw: ") + e.what()); throw Abort(); }
        R->failure_seen = R->gave_up = true;
        check(e.status >= FWA_ERR_INVALID_ARG && e.status <= FWA_ERR_UNSUPPORTED, std::string("the mirror threw status ") + std::to_string(e.status));
        check(names_step(e.what(), sim::fired_name(), hipGetErrorName(sim::fired_error())) ||
                  names_step(fwa_last_error_string(nullptr), sim::fired_name(), hipGetErrorName(sim::fired_error())),
              "the mirror threw at " + sim::fired_name() + " with '" + e.what() + "'");
    }
    check(sim::rccl_pending() == 0 && sim::rccl_live() == 0, "operations or communicators are left after the mirror's destructors");
}

// ================================================ the framed plans ================================================
// One plan: describe, create, the getters against the frame rule restated here, two execs, the grid the launcher saw, and every byte
// of dst written exactly once.  A source above 1 MiB is not uploaded but marked written, as an upload would.
void stft_case(fwa_ctx *ctx, fwa_stream *s, int32_t output, bool windowed, uint32_t n, uint32_t hop, uint64_t L, uint64_t signals)
{
    const std::string tag = "framed n " + std::to_string(n) + " hop " + std::to_string(hop) + " L " + std::to_string(L) + " x" + std::to_string(signals) +
                            (output == FWT_POWER ? " power" : " spectrum") + (windowed ? " windowed" : "");
    const uint64_t F = 1 + (L - n) / hop, frames = F * signals, row = (output == FWT_POWER ? 4ull : 8ull) * (n / 2 + 1);
    const uint64_t per_wg = n <= 64 ? 256 : 16, grid = (frames + per_wg - 1) / per_wg;
    fwa_buf *src = new_buf(ctx, 4 * L * signals), *win = windowed ? new_buf(ctx, 4ull * n) : nullptr, *dst = new_buf(ctx, frames * row);
    for (fwa_buf *b : {src, win}) {
        if (!b) continue;
        if (fwa_buf_size(b) <= (1u << 20)) {
            std::vector<char> host(fwa_buf_size(b), 1);
            call("fwa_buf_upload", ctx, [&] { return fwa_buf_upload(b, 0, host.data(), host.size(), nullptr); });
        } else sim::mark_written(fwa_buf_device_ptr(b), fwa_buf_size(b));
    }
    call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
    uint64_t d_frames = 0, d_blocks = 0;
    int32_t d_per = 0;
    call("fwt_describe", nullptr, [&] { return fwt_describe(n, hop, L, signals, &d_frames, nullptr, nullptr, &d_per, &d_blocks); });
    check(d_frames == F && d_blocks == grid && (uint64_t)d_per == per_wg, tag + ": fwt_describe differs from the frame rule");
    fwt_plan *p = nullptr;
    create("fwt_plan_create", ctx, &p, [&] { return fwt_plan_create(ctx, output, n, hop, L, src, win, dst, &p); });
    auto get = [&](const char *key) {
        int64_t v = -1;
        check(fwt_plan_get_i64(p, key, &v) == FWA_OK, tag + ": fwt_plan_get_i64 " + key);
        return (uint64_t)v;
    };
    check(get("frames_per_signal") == F && get("signals") == signals && get("frames") == frames && get("blocks") == grid && get("frames_per_block") == per_wg &&
              get("launches_per_exec") == 1 && get("windowed") == (windowed ? 1u : 0u),
          tag + ": the plan's getters differ from the frame rule");
    for (int i = 0; i < 2; ++i) {
        exec_checked("fwt_plan_exec", ctx, s, 1, [&] { return fwt_plan_exec(p, s); });
        check(sim::last_grid() == grid, tag + ": the launcher saw a grid of " + std::to_string(sim::last_grid()) + ", fwt_describe says " + std::to_string(grid));
        written_once(sim::ops().size() - 1, dev_ptr(dst), dev_ptr(dst) + frames * row, 0, 0, tag);  // the launch alone
    }
    call("fwt_plan_destroy", ctx, [&] { return fwt_plan_destroy(p); });
    call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
    for (fwa_buf *b : {src, win, dst}) call("fwa_buf_free", ctx, [&] { return fwa_buf_free(b); });
}
// frames beyond whole workgroups: 300 = 256 + 44 up to n = 64, 37 = 2 x 16 + 5 from 128 on
uint64_t stft_frames(uint32_t n) { return n <= 64 ? 300 : 37; }
// both outputs, windowed and rectangular, hop 1, 3, n/2, n, n + 5, a signal whose last frame ends exactly at its end and one a float longer (both
// parities of L), one signal and three
void stft_clean(uint32_t n)
{
    fwa_ctx *ctx = new_ctx();
    fwa_stream *s = new_stream(ctx);
    std::set<uint32_t> hops;
    for (uint32_t hop : {1u, 3u, n / 2, n, n + 5}) hops.insert(hop);
    for (int32_t output : {FWT_SPECTRUM, FWT_POWER})
        for (int windowed = 0; windowed < 2; ++windowed)
            for (uint32_t hop : hops)
                for (uint64_t tail = 0; tail < 2; ++tail)
                    for (uint64_t signals : {1ull, 3ull}) stft_case(ctx, s, output, windowed != 0, n, hop, n + (uint64_t)hop * (stft_frames(n) - 1) + tail, signals);
    call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}
void stft_few(bool large)
{
    fwa_ctx *ctx = new_ctx();
    fwa_stream *s = new_stream(ctx);
    const uint32_t a = large ? 128 : 2, b = large ? 4096 : 64;
    stft_case(ctx, s, FWT_SPECTRUM, true, a, 1, a + stft_frames(a) - 1, 3);
    stft_case(ctx, s, FWT_POWER, false, a, a + 5, a + (uint64_t)(a + 5) * (stft_frames(a) - 1) + 1, 1);
    stft_case(ctx, s, FWT_POWER, true, b, b / 2, b + (uint64_t)(b / 2) * (stft_frames(b) - 1), 3);
    stft_case(ctx, s, FWT_SPECTRUM, false, b, b, (uint64_t)b * stft_frames(b) + 1, 1);
    call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}
void stft_past_4gib()
{
    fwa_ctx *ctx = new_ctx();
    fwa_stream *s = new_stream(ctx);
    stft_case(ctx, s, FWT_POWER, true, 4096, 4096, (1ull << 30) + 4096, 1);    // src: 4 GiB + 16 KiB, its last frame at the very end
    stft_case(ctx, s, FWT_SPECTRUM, false, 4096, 1, 4096 + 270000 - 1, 1);   // dst: 270 000 rows of 16 392 bytes
    stft_case(ctx, s, FWT_SPECTRUM, true, 2, 2, 1ull << 29, 2);              // both, from the one-frame-per-thread kernel: 2^29 rows of 16 bytes
    call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
}

void build_scenarios()
{
    static const char *kinds[] = {"forward", "inverse", "onlyinverse", "normalize"};
    const std::pair<uint32_t, uint64_t> shapes[] = {{1u, 5}, {64u, 131}, {512u, 19}, {8192u, 3}, {1u << 16, 9}, {1u << 17, 9}, {1u << 20, 5},
                                                    {1u << 20, 40}, {1u << 22, 2}, {1u << 24, 2}};
    for (const auto &sh : shapes)
        for (int32_t k = FWA_FORWARD; k <= FWA_NORMALIZE; ++k)
            add(std::string("life ") + kinds[k] + " n=" + std::to_string(sh.first) + " x" + std::to_string(sh.second), sh.first,
                [=] { life_cycle(k, sh.first, sh.second); });
    // tests/test_gpu_retune.py's sequence at 2^16 x 9
    add("retune 2^16: group, streams, group, factors, path 2", 1u << 16,
        [] { retune(FWA_FORWARD, 1u << 16, 9, {{"group", 2}, {"streams", 2}, {"group", 2}, {"factors", -1}, {"path", 2}}); });
    add("retune 2^16: group, streams, factors", 1u << 16, [] { retune(FWA_FORWARD, 1u << 16, 9, {{"group", 2}, {"streams", 2}, {"factors", -1}}); });
    // the 2^20 forms
    add("retune 2^20: factors 1024x1024, 2048x512", 1u << 20,
        [] { retune(FWA_FORWARD, 1u << 20, 40, {{"factors", 10 | (10 << 8)}, {"factors", 11 | (9 << 8)}, {"group", 3}, {"streams", 3}}); });
    add("retune 2^20: factors 64x128x128", 1u << 20, [] { retune(FWA_INVERSE_SCALED, 1u << 20, 40, {{"factors", 6 | (7 << 8) | (7 << 16)}, {"streams", 2}}); });
    add("retune 2^20: path 1 -> 5 -> 1, ring_rotate", 1u << 20,
        [] { retune(FWA_FORWARD, 1u << 20, 40, {{"path", 5}, {"depth", 4}, {"ring_slots", 9}, {"wgs", 256}, {"path", 1}, {"ring_rotate", 2}, {"group", 4}, {"streams", 2}}); });
    add("retune 2^20: path 5, depth, ring_slots, wgs", 1u << 20,
        [] { retune(FWA_INVERSE_SCALED, 1u << 20, 40, {{"path", 5}, {"ring_slots", 20}, {"depth", 16}, {"wgs", 128}}); });
    add("retune 512: small_reg 3", 512, [] { retune(FWA_FORWARD, 512, 19, {{"small_reg", 3}}); });
    // the literal path forced on plans whose cached tables have no n/2 table
    add("path 2: forward, even log2 n", 1u << 16, [] { retune(FWA_FORWARD, 1u << 16, 9, {{"path", 2}}); });
    add("path 2: forward, odd log2 n", 1u << 17, [] { retune(FWA_FORWARD, 1u << 17, 9, {{"path", 2}}); });
    add("path 2: onlyinverse", 1u << 16, [] { retune(FWA_INVERSE_UNSCALED, 1u << 16, 9, {{"path", 2}}); });
    add("path 2: forward, n = 64", 64, [] { retune(FWA_FORWARD, 64, 131, {{"path", 2}}); });
    add("plan cache and ring pool", 1u << 20, cache_and_pool);
    add("buffers", 0, buffers);
    add("streams and events", 0, streams_and_events);
    add("destroy in flight: owned stream", 1u << 16, [] { destroy_in_flight(0); });
    add("destroy in flight: wrapped stream", 1u << 16, [] { destroy_in_flight(1); });
    add("destroy in flight: destroyed stream", 1u << 16, [] { destroy_in_flight(2); });
    add("destroy in flight: wrapped stream, during a capture", 1u << 16, [] { destroy_in_flight(3); });
    add("side libraries: small", 128, [] { side_libraries(false); });
    add("side libraries: large", 4096, [] { side_libraries(true); });
    // The communicators.  The audits are sweeps (thousands of collectives each): the clean run has them, the fault sweep takes the single
    // cases below them instead -- every world size, with and without an empty slab, every order, the root first, last and in between.
    constexpr uint64_t SWEEP = ~0ull;
    for (int world = 1; world <= 8; ++world) add("comm audit: world " + std::to_string(world), SWEEP, [=] { comm_audit(world); });
    for (int world = 1; world <= 8; ++world) {
        const uint64_t batch = world % 2 ? 3 * (uint64_t)world + 2 : (uint64_t)world - 1;  // even worlds: the last rank's slab is empty
        const int root = world / 2, order = world % 3;
        add("comm: scatter, exec, gather, world " + std::to_string(world) + " x" + std::to_string(batch), 512, [=] { comm_small(world, 512, batch, root, order, world == 5); });
    }
    add("comm: scatter, exec, gather, world 2, n=2^20", 1u << 20, [] { comm_small(2, 1u << 20, 5, 1, 0, false); });
    for (int world : {2, 3, 8}) add("comm: sendrecv ring, world " + std::to_string(world), 0, [=] { comm_ring(world); });
    add("comm: sendrecv forms and refusals", 0, comm_forms);
    add("comm: lifetimes and foreign handles", 0, comm_lifetimes);
    add("comm: the documented hazard", 0, comm_documented_hazard);
    add("comm: C++ mirror, world 3", 512, comm_mirror);
    // The framed plans.  The products are sweeps too (80 plans each); the fault sweep takes the two scenarios of a few plans each below them,
    // which reach both kernels, both outputs, both window forms, a partial workgroup and a hop beyond the frame, and the plans past 4 GiB.
    for (uint32_t n : {2u, 64u, 128u, 4096u}) add("framed plans: n=" + std::to_string(n) + ", every form", SWEEP, [=] { stft_clean(n); });
    add("framed plans: a few, n = 2 and 64", 64, [] { stft_few(false); });
    add("framed plans: a few, n = 128 and 4096", 4096, [] { stft_few(true); });
    add("framed plans: src and dst past 4 GiB", 4096, stft_past_4gib);
}

// one run of a scenario on a fresh fake; returns the violations it ends with (the audit's included)
struct Outcome { uint64_t violations, calls; bool aborted; std::vector<std::vector<std::string>> execs; };
Outcome run_scenario(const Scenario &sc, int64_t arm_k, const std::vector<std::vector<std::string>> *clean)
{
    Run run;
    run.tolerant = arm_k >= 0; run.name = sc.name + (arm_k >= 0 ? " [call " + std::to_string(arm_k) + " fails]" : "");
    R = &run;
    sim::reset();
    set_ipc_mode(arm_k >= 0 ? (int)(arm_k % 3) : 0);
    if (arm_k >= 0) sim::arm(arm_k);
    else sim::arm(-1);
    bool aborted = false;
    try { sc.run(); } catch (const Abort &) { aborted = true; }
    (void)sim::rccl_group_closed("the scenario");
    const uint64_t calls = sim::injectable_calls();
    if (arm_k >= 0) {
        check(sim::fired(), "the armed call was never reached");
        if (g_verbose) std::printf("  k=%lld %s%s\n", (long long)arm_k, sim::fired_name().c_str(), run.failure_seen ? " -> status" : "");
    }
    if (!aborted) {
        sim::audit_leaks();
        if (clean) {
            check(run.gave_up ? run.execs.size() <= clean->size() : run.execs.size() == clean->size(),
                  "the run made " + std::to_string(run.execs.size()) + " execs, the clean run " + std::to_string(clean->size()));
            for (size_t i = 0; i < run.execs.size() && i < clean->size(); ++i)
                if (run.execs[i] != (*clean)[i]) {
                    std::string d;
                    for (size_t j = 0; j < run.execs[i].size() || j < (*clean)[i].size(); ++j) {
                        const std::string x = j < run.execs[i].size() ? run.execs[i][j] : "(none)", y = j < (*clean)[i].size() ? (*clean)[i][j] : "(none)";
                        if (x != y) { d = "launch " + std::to_string(j) + ": '" + x + "' against '" + y + "'"; break; }
                    }
                    check(false, "exec " + std::to_string(i) + " after the failure differs from the clean run: " + d);
                }
        }
    }
    Outcome o{sim::violations_total(), calls, aborted, run.execs};
    if (o.violations) {
        std::printf("VIOLATIONS in %s:\n", run.name.c_str());
        for (const std::string &l : sim::violation_log()) std::printf("    %s\n", l.c_str());
    }
    R = nullptr;
    return o;
}

// The table holds the whole expected set (declared in main before anything runs), so a function that no scenario reaches is a
// row with zero calls, and the condition fails on it.
void print_coverage(uint64_t *runtime_failed, uint64_t *launchers_failed, uint64_t *never)
{
    *runtime_failed = *launchers_failed = *never = 0;
    std::printf("coverage: injectable function, calls seen, times it was the failing call\n");
    for (const sim::Coverage &c : sim::coverage()) {
        std::printf("  %-34s %9llu %6llu%s\n", c.name.c_str(), (unsigned long long)c.calls, (unsigned long long)c.failed, c.failed ? "" : "   <-- never failed");
        if (!c.failed) ++*never;
        else ++*(c.name.compare(0, 3, "hip") == 0 || c.name.compare(0, 4, "nccl") == 0 ? runtime_failed : launchers_failed);
    }
    std::printf("not injectable (the error reporters themselves):");
    for (const std::string &s : sim::not_injectable()) std::printf(" %s", s.c_str());
    std::printf(" ncclGetErrorString\nruntime functions include the seven injectable entry points of the simulated RCCL (nccl*)\n");
}

// ---- modes ----
// two ranks of one id on devices 0 and 1 with 4 KiB each (the first written), for the self-test
struct TwoRanks {
    ncclComm_t comm[2] = {nullptr, nullptr};
    void *buf[2] = {nullptr, nullptr};
    TwoRanks()
    {
        ncclUniqueId id;
        (void)fake_rccl_get_unique_id(&id);
        for (int r = 0; r < 2; ++r) {
            (void)hipSetDevice(r);
            (void)fake_rccl_comm_init_rank(&comm[r], 2, id, r);
            (void)hipMalloc(&buf[r], 4096);
        }
        sim::mark_written(buf[0], 4096);
    }
    void exchange(const void *from, size_t sent, void *to, size_t expected)  // rank 0 sends, rank 1 receives
    {
        for (int r = 0; r < 2; ++r) {
            (void)hipSetDevice(r);
            (void)fake_rccl_group_start();
            if (r == 0) (void)fake_rccl_send(from, sent, ncclInt8, 1, comm[0], nullptr);
            else (void)fake_rccl_recv(to, expected, ncclInt8, 0, comm[1], nullptr);
            (void)fake_rccl_group_end();
        }
    }
    ~TwoRanks()
    {
        for (int r = 0; r < 2; ++r) {
            (void)hipSetDevice(r);
            (void)fake_rccl_comm_destroy(comm[r]);
            (void)hipFree(buf[r]);
        }
    }
};

int selftest()
{
    struct Case { const char *name; int kind; std::function<void()> misuse; };
    const Case cases[] = {
        {"double hipFree", sim::V_DOUBLE_FREE, [] {
             void *p = nullptr;
             (void)hipMalloc(&p, 4096);
             (void)hipFree(p);
             (void)hipFree(p);
         }},
        {"launch 8 bytes past an allocation", sim::V_OUT_OF_BOUNDS, [] {
             void *p = nullptr;
             (void)hipMalloc(&p, 4096);
             (void)sim::launch("misuse", nullptr, {}, {sim::Region{static_cast<char *>(p) + 8, 4096, {}}});
             (void)hipFree(p);
         }},
        {"read of an unwritten table", sim::V_UNWRITTEN_READ, [] {
             void *tw = nullptr, *out = nullptr;
             (void)hipMalloc(&tw, 4096);
             (void)hipMalloc(&out, 4096);
             (void)sim::launch("misuse", nullptr, {sim::Region{tw, 4096, {}}}, {sim::Region{out, 4096, {}}});
             (void)hipFree(tw);
             (void)hipFree(out);
         }},
        {"overlapping ring writes on two streams, no event", sim::V_HAZARD, [] {
             void *ring = nullptr;
             hipStream_t a = nullptr, b = nullptr;
             (void)hipMalloc(&ring, 1 << 20);
             (void)hipStreamCreateWithFlags(&a, hipStreamNonBlocking);
             (void)hipStreamCreateWithFlags(&b, hipStreamNonBlocking);
             (void)sim::launch("misuse a", a, {}, {sim::Region{ring, 1 << 19, {}}});
             (void)sim::launch("misuse b", b, {}, {sim::Region{static_cast<char *>(ring) + (1 << 19) - 8, 1 << 19, {}}});
             (void)hipStreamDestroy(a);
             (void)hipStreamDestroy(b);
             (void)hipFree(ring);
         }},
        {"one leaked event", sim::V_LEAK, [] {
             hipEvent_t e = nullptr;
             (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
         }},
        // the simulated RCCL, called as comm.cpp calls it
        {"a send nobody receives", sim::V_UNMATCHED, [] {
             TwoRanks t;
             (void)hipSetDevice(0);
             (void)fake_rccl_group_start();
             (void)fake_rccl_send(t.buf[0], 64, ncclInt8, 1, t.comm[0], nullptr);
             (void)fake_rccl_group_end();
             (void)sim::rccl_complete("misuse");
         }},
        {"64 bytes sent, 32 expected", sim::V_SIZE_MISMATCH, [] {
             TwoRanks t;
             t.exchange(t.buf[0], 64, t.buf[1], 32);
         }},
        {"two ranks of one id on one device", sim::V_COMM_INIT, [] {
             ncclUniqueId id;
             ncclComm_t a = nullptr, b = nullptr;
             (void)fake_rccl_get_unique_id(&id);
             (void)hipSetDevice(0);
             (void)fake_rccl_comm_init_rank(&a, 2, id, 0);
             (void)fake_rccl_comm_init_rank(&b, 2, id, 1);
             (void)fake_rccl_comm_destroy(a);
         }},
        {"a group left open", sim::V_GROUP_OPEN, [] {
             (void)fake_rccl_group_start();
             (void)sim::rccl_group_closed("misuse");
         }},
        {"a receive into memory of another device", sim::V_OUT_OF_BOUNDS, [] {
             TwoRanks t;
             t.exchange(t.buf[0], 64, static_cast<char *>(t.buf[0]) + 1024, 64);  // rank 1 names a range of device 0
         }},
        {"a framed launch whose last frame runs 4 bytes past src", sim::V_OUT_OF_BOUNDS, [] {
             void *src = nullptr, *dst = nullptr;
             const uint64_t n = 64, hop = 32, L = 64 + 32 * 9;  // 10 frames
             (void)hipMalloc(&src, 4 * L - 4);
             (void)hipMalloc(&dst, 10 * 8 * (n / 2 + 1));
             sim::mark_written(src, 4 * L - 4);
             (void)fwt::launch_stft((uint32_t)n, (uint32_t)hop, L, 1, false, static_cast<const float *>(src), nullptr, static_cast<float *>(dst), nullptr);
             (void)hipFree(src);
             (void)hipFree(dst);
         }},
    };
    int bad = 0, n = 0;
    Run run;
    run.name = "selftest";
    R = &run;
    for (const char *n : {"misuse", "misuse a", "misuse b", "use a", "use b"}) sim::declare(n, sim::FN_LAUNCH);  // the self-test's own launches
    for (const Case &c : cases) {
        sim::reset();
        c.misuse();
        sim::audit_leaks();
        const bool ok = sim::violations(c.kind) == 1 && sim::violations_total() == 1;
        std::printf("  %-50s -> %s x%llu, %llu in all: %s\n", c.name, sim::kind_name(c.kind), (unsigned long long)sim::violations(c.kind),
                    (unsigned long long)sim::violations_total(), ok ? "reported" : "MISSED");
        bad += !ok;
        ++n;
    }
    // and the ordered forms of the same uses are clean: an event between the two writers, a table that was uploaded
    sim::reset();
    {
        void *ring = nullptr;
        hipStream_t a = nullptr, b = nullptr;
        hipEvent_t e = nullptr;
        char host[64] = {};
        (void)hipMalloc(&ring, 1 << 20);
        (void)hipMemcpy(ring, host, 64, hipMemcpyHostToDevice);
        (void)hipStreamCreateWithFlags(&a, hipStreamNonBlocking);
        (void)hipStreamCreateWithFlags(&b, hipStreamNonBlocking);
        (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
        (void)sim::launch("use a", a, {sim::Region{ring, 64, {}}}, {sim::Region{ring, 1 << 19, {}}});
        (void)hipEventRecord(e, a);
        (void)hipStreamWaitEvent(b, e, 0);
        (void)sim::launch("use b", b, {}, {sim::Region{static_cast<char *>(ring) + (1 << 19) - 8, 1 << 19, {}}});
        (void)hipEventDestroy(e);
        (void)hipStreamDestroy(a);
        (void)hipStreamDestroy(b);
        (void)hipFree(ring);
        {   // a matched exchange of equal sizes between the two devices, receive posted first
            TwoRanks t;
            (void)hipSetDevice(1);
            (void)fake_rccl_group_start();
            (void)fake_rccl_recv(t.buf[1], 64, ncclInt8, 0, t.comm[1], nullptr);
            (void)fake_rccl_group_end();
            (void)hipSetDevice(0);
            (void)fake_rccl_group_start();
            (void)fake_rccl_send(t.buf[0], 64, ncclInt8, 1, t.comm[0], nullptr);
            (void)fake_rccl_group_end();
            (void)sim::rccl_complete("use");
            (void)sim::rccl_group_closed("use");
            (void)hipSetDevice(0);
        }
        sim::audit_leaks();
        const bool ok = sim::violations_total() == 0;
        std::printf("  %-50s -> %llu violations: %s\n", "the ordered forms of the same uses", (unsigned long long)sim::violations_total(), ok ? "clean" : "FALSE ALARM");
        bad += !ok;
    }
    R = nullptr;
    sim::reset();
    std::printf("host_faults selftest: %d of %d misuse kinds reported, each as its own kind: %s\n", n - bad, n, bad ? "FAILED" : "ok");
    return bad != 0;
}

int clean_audit()
{
    uint64_t bad = 0, execs = 0, alive = 0;
    for (const Scenario &sc : g_scenarios) {
        const Outcome o = run_scenario(sc, -1, nullptr);
        const sim::Live l = sim::live();
        std::printf("  %-58s %5llu calls %3zu execs, live: %llu allocations %llu pinned %llu streams %llu events\n", sc.name.c_str(), (unsigned long long)o.calls,
                    o.execs.size(), (unsigned long long)l.allocs, (unsigned long long)l.pinned, (unsigned long long)l.streams, (unsigned long long)l.events);
        bad += o.violations + o.aborted;
        alive += l.allocs + l.pinned + l.streams + l.events + sim::rccl_live() + sim::rccl_pending();
        execs += o.execs.size();
    }
    sim::reset();
    std::printf("host_faults clean: %zu scenarios, %llu execs, %llu violations, %llu live resources: %s\n", g_scenarios.size(), (unsigned long long)execs,
                (unsigned long long)bad, (unsigned long long)alive, bad || alive ? "FAILED" : "ok");
    return bad != 0 || alive != 0;
}

int geometry_sweep()
{
    uint64_t bad = 0, combos = 0, launches = 0;
    Scenario sc{"geometry", 0, [&] {
        fwa_ctx *ctx = new_ctx();
        fwa_stream *s = new_stream(ctx);
        for (uint32_t lg = 16; lg <= 30; ++lg) {
            std::set<uint64_t> batches;  // capped so that n x batch <= 2^32 samples; batches that meet at the cap run once
            for (uint64_t batch : {1ull, 3ull, 17ull, 40ull}) batches.insert(batch < ((1ull << 32) >> lg) ? batch : (1ull << 32) >> lg);
            for (uint64_t b : batches) {
                fwa_buf *src = new_buf(ctx, (8ull << lg) * b);
                call("fwa_fill_synthetic", ctx, [&] { return fwa_fill_synthetic(src, 1, 0, 1u << lg, 1.0f, nullptr); });
                call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
                for (int64_t group : {1, 2, 0})
                    for (int64_t streams : {1, 2, 3}) {
                        R->name = "geometry 2^" + std::to_string(lg) + " x" + std::to_string(b) + " group " + std::to_string(group) + " streams " + std::to_string(streams);
                        fwa_plan *p = new_plan(ctx, lg % 3 == 0 ? FWA_INVERSE_SCALED : FWA_FORWARD, 1u << lg, src, nullptr);
                        if (group) set(p, ctx, "group", group);
                        set(p, ctx, "streams", streams);
                        const size_t first = sim::ops().size();
                        exec(p, ctx, s);
                        launches += sim::ops().size() - first;
                        call("fwa_plan_destroy", ctx, [&] { return fwa_plan_destroy(p); });
                        ++combos;
                    }
                call("fwa_ctx_synchronize", ctx, [&] { return fwa_ctx_synchronize(ctx); });
                call("fwa_buf_free", ctx, [&] { return fwa_buf_free(src); });
            }
        }
        call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
        call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
    }};
    const Outcome o = run_scenario(sc, -1, nullptr);
    bad = o.violations + o.aborted;
    const sim::Live l = sim::live();
    bad += l.allocs + l.pinned + l.streams + l.events;
    // the framed plans: every length, hop 1, 2, 3, n/4, n/2, n, n + 5 (those that repeat or fall below 1 once), a signal of one frame, of one
    // frame and a float, and of whole and partial workgroups of frames with half a hop left over, one signal and three
    uint64_t framed = 0;
    Scenario fr{"framed geometry", 0, [&] {
        fwa_ctx *ctx = new_ctx();
        fwa_stream *s = new_stream(ctx);
        for (uint32_t n = 2; n <= 4096; n *= 2) {
            std::set<uint32_t> hops;
            for (uint32_t hop : {1u, 2u, 3u, n / 4, n / 2, n, n + 5})
                if (hop >= 1) hops.insert(hop);
            for (uint32_t hop : hops)
                for (uint64_t L : {(uint64_t)n, (uint64_t)n + 1, n + (uint64_t)hop * (stft_frames(n) - 1) + hop / 2})
                    for (uint64_t signals : {1ull, 3ull}) {
                        R->name = "framed geometry";
                        stft_case(ctx, s, framed % 2 ? FWT_POWER : FWT_SPECTRUM, framed % 4 < 2, n, hop, L, signals);
                        ++framed;
                    }
        }
        call("fwa_stream_destroy", ctx, [&] { return fwa_stream_destroy(s); });
        call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
    }};
    const Outcome of = run_scenario(fr, -1, nullptr);
    bad += of.violations + of.aborted;
    const sim::Live lf = sim::live();
    const uint64_t alive = l.allocs + l.pinned + l.streams + l.events + lf.allocs + lf.pinned + lf.streams + lf.events;
    bad += lf.allocs + lf.pinned + lf.streams + lf.events;
    sim::reset();
    std::printf("host_faults geometry: %llu plans of 2^16 .. 2^30, %llu launches, %llu framed plans of 2 .. 4096, %llu violations, %llu live resources: %s\n",
                (unsigned long long)combos, (unsigned long long)launches, (unsigned long long)framed, (unsigned long long)bad, (unsigned long long)alive, bad ? "FAILED" : "ok");
    return bad != 0;
}

int fault_sweep()
{
    uint64_t bad = 0, points = 0, n_sc = 0;
    for (const Scenario &sc : g_scenarios) {
        if (sc.max_n > (1u << 20)) continue;
        const Outcome clean = run_scenario(sc, -1, nullptr);
        bad += clean.violations + clean.aborted;
        uint64_t sc_bad = 0;
        for (uint64_t k = 0; k < clean.calls; ++k) {  // every index, none skipped
            const Outcome o = run_scenario(sc, (int64_t)k, &clean.execs);
            sc_bad += o.violations + o.aborted;
            ++points;
        }
        std::printf("  %-58s %5llu injection points, %llu violations\n", sc.name.c_str(), (unsigned long long)clean.calls, (unsigned long long)sc_bad);
        bad += sc_bad;
        ++n_sc;
    }
    // the coverage condition: every function of the expected set has been the failing call (with --only it fails, as it should)
    uint64_t rt = 0, ln = 0, never = 0;
    print_coverage(&rt, &ln, &never);
    sim::reset();
    std::printf("host_faults faults: %llu scenarios, %llu injection points, %llu violations, failing call at least once: %llu runtime functions and "
                "%llu launchers and setups, %llu never: %s\n", (unsigned long long)n_sc, (unsigned long long)points, (unsigned long long)bad,
                (unsigned long long)rt, (unsigned long long)ln, (unsigned long long)never, bad || never ? "FAILED" : "ok");
    return bad != 0 || never != 0;
}

// The simulated RCCL must be the librccl.so.1 of this process and an installed one must never load (it would bring a real HIP runtime
// with it).  The first directory of LD_LIBRARY_PATH that holds the name must hold a small file; that file is loaded here, by its path,
// and must carry the fake's marker.  Its soname is the name comm.cpp asks for, so comm.cpp's own dlopen finds it loaded.
bool load_fake_rccl(bool *has_recv)
{
    const char *path = std::getenv("LD_LIBRARY_PATH");
    std::string dirs = path ? path : "", file;
    for (size_t at = 0; at <= dirs.size() && file.empty();) {
        const size_t end = std::min(dirs.find(':', at), dirs.size());
        const std::string candidate = dirs.substr(at, end - at) + "/librccl.so.1";
        struct stat st;
        if (end > at && stat(candidate.c_str(), &st) == 0) {
            if (st.st_size > (1 << 20)) { std::printf("host_faults: %s is no simulated RCCL (%lld bytes): not loaded\n", candidate.c_str(), (long long)st.st_size); return false; }
            file = candidate;
        }
        at = end + 1;
    }
    if (file.empty()) { std::printf("host_faults: no librccl.so.1 in LD_LIBRARY_PATH: build tools/host_sim/fake_rccl.cpp with -DFAKE_RCCL_SHARED and point it there\n"); return false; }
    void *so = dlopen(file.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!so) { std::printf("host_faults: dlopen(%s): %s\n", file.c_str(), dlerror()); return false; }
    if (!dlsym(so, "fake_rccl_marker")) { std::printf("host_faults: %s is not the simulated RCCL\n", file.c_str()); return false; }
    void *again = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    if (again != so) { std::printf("host_faults: the name librccl.so.1 does not lead to %s\n", file.c_str()); return false; }
    *has_recv = dlsym(so, "ncclRecv") != nullptr;
    return true;
}

// against the stub without ncclRecv: what can be reached without a communicator answers FWA_ERR_UNSUPPORTED and names the symbol; the
// pure host logic still works
int stub_run()
{
    Run run;
    run.name = "stub";
    R = &run;
    sim::reset();
    auto unsupported = [&](const char *what, int32_t st, const fwa_ctx *ctx) {
        const std::string msg = fwa_last_error_string(ctx);
        check(st == FWA_ERR_UNSUPPORTED && msg.find("ncclRecv") != std::string::npos, std::string(what) + " returned " + std::to_string(st) + " ('" + msg + "')");
        std::printf("  %-24s -> %d %s\n", what, st, msg.c_str());
    };
    uint8_t id[FWA_COMM_ID_BYTES] = {};
    unsupported("fwa_comm_unique_id", fwa_comm_unique_id(id), nullptr);
    fwa_ctx *ctx = new_ctx();
    fwa_comm *c = reinterpret_cast<fwa_comm *>(uintptr_t(16));
    unsupported("fwa_comm_create", fwa_comm_create(ctx, id, 2, 0, &c), ctx);
    check(c == nullptr, "a refused fwa_comm_create left *out set");
    check(fwa_comm_destroy(nullptr) == FWA_OK, "fwa_comm_destroy(NULL)");
    check(sim::rccl_calls() == 0, "an entry point of the stub was called");
    uint64_t first = 0, count = 0, off[3], len[3];
    int32_t peer[3], np = 0;
    check(fwa_slab(11, 1, 3, &first, &count) == FWA_OK && first == 4 && count == 4, "fwa_slab without RCCL");
    check(fwa_comm_pieces(11, 8, 1, 1, 3, off, len, peer, &np) == FWA_OK && np == 3 && off[2] == 8 * 64 && len[2] == 3 * 64 && peer[1] == -1 && peer[2] == 2,
          "fwa_comm_pieces without RCCL");
    call("fwa_ctx_destroy", nullptr, [&] { return fwa_ctx_destroy(ctx); });
    sim::audit_leaks();
    const uint64_t bad = sim::violations_total();
    for (const std::string &l : sim::violation_log()) std::printf("    %s\n", l.c_str());
    R = nullptr;
    sim::reset();
    std::printf("host_faults stub: librccl.so.1 without ncclRecv: fwa_comm_unique_id and fwa_comm_create answer FWA_ERR_UNSUPPORTED and name the symbol, "
                "fwa_slab and fwa_comm_pieces work, %llu violations: %s\n", (unsigned long long)bad, bad ? "FAILED" : "ok");
    return bad != 0;
}

}  // namespace

int main(int argc, char **argv)
{
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    build_scenarios();
    sim::declare_runtime();
    sim::declare_rccl();
    sim::declare_launchers();
    std::string mode = argc > 1 ? argv[1] : "";
    for (int i = 2; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--verbose")) g_verbose = true;
        else if (!std::strcmp(argv[i], "--only") && i + 1 < argc) {
            std::vector<Scenario> keep;
            for (const Scenario &s : g_scenarios)
                if (s.name.find(argv[i + 1]) != std::string::npos) keep.push_back(s);
            g_scenarios = keep;
            ++i;
        }
    }
    if (mode == "--selftest") return selftest();
    bool has_recv = false;
    if (mode == "--clean" || mode == "--faults" || mode == "--stub") {
        if (!load_fake_rccl(&has_recv)) return 3;
        if (has_recv != (mode != "--stub")) {
            std::printf("host_faults: %s needs the simulated RCCL %s ncclRecv\n", mode.c_str(), mode == "--stub" ? "without" : "with");
            return 3;
        }
    }
    if (mode == "--stub") return stub_run();
    if (mode == "--clean") return clean_audit();
    if (mode == "--geometry") return geometry_sweep();
    if (mode == "--faults") return fault_sweep();
    std::printf("usage: host_faults --selftest | --clean | --geometry | --faults | --stub [--only NAME] [--verbose]\n");
    return 2;
}
