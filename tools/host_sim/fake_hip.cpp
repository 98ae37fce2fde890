// fake_hip.cpp -- a simulated HIP runtime for the library's host layer: exactly the runtime entry points that the host
// objects (fft_wgpu_amd/csrc/*.cpp and the four side-library hosts) leave undefined, with the real hip_runtime_api.h for
// types and signatures.  A missing entry point is a link error: that is the completeness check.
//
// Eight devices.  Device memory is address space only: hipMalloc is a bump allocator over a range nothing maps, every
// allocation keeps its device, base, size, liveness, the set of bytes written so far and the accesses made to it.  Streams
// and events are counted handles; every stream carries a vector clock, hipEventRecord snapshots it, hipStreamWaitEvent
// merges the snapshot, the synchronising calls merge into the host's clock, and the host's clock goes into every
// operation enqueued afterwards.  Two accesses are ordered when the later one's clock has reached the earlier one's tick.
#include "fake_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

namespace sim {
namespace {

constexpr int N_DEV = 8;
constexpr uint64_t dev_base(int d) { return 0x200000000000ull + (uint64_t)d * 0x400000000000ull; }  // 64 TiB of addresses each, never mapped
constexpr uint64_t HBM_BYTES = 288ull << 30;
constexpr uint64_t ALIGN = 256, GUARD = 4096;

using VC = std::vector<uint64_t>;
void merge(VC &into, const VC &from)
{
    if (into.size() < from.size()) into.resize(from.size(), 0);
    for (size_t i = 0; i < from.size(); ++i) into[i] = std::max(into[i], from[i]);
}
uint64_t at(const VC &v, size_t i) { return i < v.size() ? v[i] : 0; }

struct Access { uint64_t lo, hi; bool write; int sid; uint64_t tick; std::string op; };
struct Alloc {
    int dev = 0;
    uint64_t base = 0, size = 0;
    bool live = true, orphan = false;
    std::map<uint64_t, uint64_t> written;  // disjoint [lo, hi), merged
    std::vector<Access> hist;
};
struct Stream { int id = 0, dev = 0; unsigned flags = 0; bool live = true, orphan = false, capturing = false; VC vc; };
struct Event { int dev = 0; bool live = true, orphan = false, recorded = false; VC snap; };

struct Books {
    int current = 0;
    bool peer[N_DEV][N_DEV] = {};
    uint64_t bump[N_DEV] = {}, live_bytes[N_DEV] = {};
    std::map<uint64_t, Alloc> allocs;            // by base; dead ones stay (addresses are never handed out twice)
    std::map<void *, bool> pinned;               // pointer -> orphan
    std::vector<Stream> streams;                 // [0 .. N_DEV): the null streams of the devices
    std::map<hipStream_t, int> stream_of;
    std::vector<Event> events;
    std::map<hipEvent_t, int> event_of;
    VC host;
    hipError_t sticky = hipSuccess;
    Counters cnt{0, 0, 0, 0};
    std::vector<Op> ops;
    uint64_t viol[V_KINDS] = {};
    std::vector<std::string> log;
    // injection
    int64_t armed_k = -1;
    hipError_t armed_err = hipSuccess, fired_err = hipSuccess;
    bool fired = false;
    std::string fired_name;
    uint64_t n_calls = 0;
    // knobs
    std::vector<float> elapsed;
    size_t elapsed_next = 0;
    float elapsed_then = 0.04f;
    uint64_t grid = 0;
};
Books *g = nullptr;
std::map<std::string, Coverage> g_cov;  // whole process

Books &B()
{
    if (!g) reset();
    return *g;
}

hipError_t err(hipError_t e)
{
    if (e != hipSuccess) B().sticky = e;
    return e;
}

hipStream_t stream_handle(int id) { return reinterpret_cast<hipStream_t>((uintptr_t)0x51000000u + (uintptr_t)id * 0x100u); }
hipEvent_t event_handle(int id) { return reinterpret_cast<hipEvent_t>((uintptr_t)0x61000000u + (uintptr_t)id * 0x100u); }

// the stream a handle names: nullptr = the null stream of the current device; unknown or dead = a violation
Stream *stream(hipStream_t h, const char *who)
{
    Books &b = B();
    if (!h) return &b.streams[(size_t)b.current];
    auto it = b.stream_of.find(h);
    if (it == b.stream_of.end()) { violation(V_DEAD_HANDLE, std::string(who) + ": unknown stream handle"); return nullptr; }
    Stream &s = b.streams[(size_t)it->second];
    if (!s.live) { violation(V_DEAD_HANDLE, std::string(who) + ": stream " + std::to_string(s.id) + " has been destroyed"); return nullptr; }
    return &s;
}
Event *event(hipEvent_t h, const char *who)
{
    Books &b = B();
    auto it = b.event_of.find(h);
    if (it == b.event_of.end()) { violation(V_DEAD_HANDLE, std::string(who) + ": unknown event handle"); return nullptr; }
    Event &e = b.events[(size_t)it->second];
    if (!e.live) { violation(V_DEAD_HANDLE, std::string(who) + ": event " + std::to_string(it->second) + " has been destroyed"); return nullptr; }
    return &e;
}

// An operation starts on s: what the host has waited for and what the null-stream rule orders come first.
uint64_t begin_op(Stream &s)
{
    Books &b = B();
    merge(s.vc, b.host);
    const bool is_null = s.id < N_DEV;
    if (is_null) {
        for (const Stream &o : b.streams)  // the legacy null stream waits for every blocking stream of its device
            if (o.id >= N_DEV && o.live && o.dev == s.dev && !(o.flags & hipStreamNonBlocking)) merge(s.vc, VC(o.vc));
    } else if (!(s.flags & hipStreamNonBlocking)) {
        merge(s.vc, VC(b.streams[(size_t)s.dev].vc));  // and a blocking stream waits for the null stream
    }
    if (s.vc.size() <= (size_t)s.id) s.vc.resize((size_t)s.id + 1, 0);
    return ++s.vc[(size_t)s.id];
}

Alloc *find_alloc(uint64_t addr)
{
    Books &b = B();
    auto it = b.allocs.upper_bound(addr);
    if (it == b.allocs.begin()) return nullptr;
    --it;
    return addr < it->second.base + it->second.size ? &it->second : nullptr;
}

// check (a): [lo, hi) inside one live allocation of device `dev`
Alloc *bounded(uint64_t lo, uint64_t hi, int dev, const std::string &who)
{
    char t[160];
    Alloc *a = find_alloc(lo);
    if (!a || hi > a->base + a->size) {
        std::snprintf(t, sizeof t, ": [%#llx, %#llx) is not inside one allocation (%lld bytes past its end)", (unsigned long long)lo,
                      (unsigned long long)hi, a ? (long long)(hi - a->base - a->size) : -1ll);
        violation(V_OUT_OF_BOUNDS, who + t);
        return nullptr;
    }
    if (!a->live) { violation(V_OUT_OF_BOUNDS, who + ": the allocation has been freed"); return nullptr; }
    if (a->dev != dev) { violation(V_OUT_OF_BOUNDS, who + ": the allocation lives on another device"); return nullptr; }
    return a;
}

// check (b): every byte of [lo, hi) written
bool is_written(const Alloc &a, uint64_t lo, uint64_t hi)
{
    auto it = a.written.upper_bound(lo);
    if (it == a.written.begin()) return false;
    --it;
    return it->first <= lo && hi <= it->second;
}
void set_written(Alloc &a, uint64_t lo, uint64_t hi)
{
    auto it = a.written.upper_bound(lo);
    if (it != a.written.begin()) {
        auto p = std::prev(it);
        if (p->second >= lo) { lo = p->first; hi = std::max(hi, p->second); it = a.written.erase(p); }
    }
    while (it != a.written.end() && it->first <= hi) { hi = std::max(hi, it->second); it = a.written.erase(it); }
    a.written[lo] = hi;
}

// check (c) and the record of the access
void access(Alloc &a, uint64_t lo, uint64_t hi, bool write, const Stream &s, uint64_t tick, const std::string &op)
{
    for (size_t i = 0; i < a.hist.size();) {
        const Access &o = a.hist[i];
        const bool overlap = o.lo < hi && lo < o.hi;
        if (overlap && (o.write || write) && o.sid != s.id && at(s.vc, (size_t)o.sid) < o.tick) {
            char t[200];
            std::snprintf(t, sizeof t, " [%#llx, %#llx) on stream %d is not ordered behind ", (unsigned long long)std::max(lo, o.lo),
                          (unsigned long long)std::min(hi, o.hi), s.id);
            violation(V_HAZARD, op + (write ? " writes" : " reads") + t + o.op + (o.write ? " (write" : " (read") + ", stream " +
                                    std::to_string(o.sid) + ")");
        }
        // an ordered access that this one covers completely says nothing a later check could not learn from this one
        const bool ordered = o.sid == s.id || at(s.vc, (size_t)o.sid) >= o.tick;
        if (overlap && ordered && lo <= o.lo && o.hi <= hi && (write || !o.write)) a.hist.erase(a.hist.begin() + (std::ptrdiff_t)i);
        else ++i;
    }
    a.hist.push_back({lo, hi, write, s.id, tick, op});
}

// one side of a copy or one range of a launch
void touch(Op &op, uint64_t lo, uint64_t hi, bool write, Stream &s, uint64_t tick)
{
    if (lo >= hi) return;
    Alloc *a = bounded(lo, hi, s.dev, op.name);
    if (!a) return;
    if (!write && !is_written(*a, lo, hi)) {
        char t[120];
        std::snprintf(t, sizeof t, " reads [%#llx, %#llx), which nothing has written completely", (unsigned long long)lo, (unsigned long long)hi);
        violation(V_UNWRITTEN_READ, op.name + t);
    }
    access(*a, lo, hi, write, s, tick, op.name);
    (write ? op.writes : op.reads).push_back({lo, hi});
}

void read_host(const void *p, size_t bytes)  // every 8-byte granule once: AddressSanitizer sees an overrun of the host side
{
    const volatile unsigned char *c = static_cast<const volatile unsigned char *>(p);
    unsigned sum = 0;
    for (size_t i = 0; i < bytes; i += 8) sum += c[i];
    if (bytes) sum += c[bytes - 1];
    (void)sum;
}

hipError_t copy(const char *name, void *dst, int dst_dev, const void *src, int src_dev, size_t bytes, hipMemcpyKind kind, hipStream_t st,
                bool sync)
{
    Books &b = B();
    Stream *s = stream(st, name);
    if (!s) return err(hipErrorInvalidHandle);
    if (s->dev != b.current) violation(V_CHECK, std::string(name) + ": the stream belongs to a device that is not current");
    Op op{name, st, s->id, begin_op(*s), {}, {}, false};
    const uint64_t d = reinterpret_cast<uint64_t>(dst), r = reinterpret_cast<uint64_t>(src);
    Stream from = *s, to = *s;  // a peer copy touches memory of two devices; ordering is the stream's either way
    from.dev = src_dev; to.dev = dst_dev;
    if (kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice) touch(op, r, r + bytes, false, from, op.tick);
    else read_host(src, bytes);
    if (kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice) {
        touch(op, d, d + bytes, true, to, op.tick);
        if (Alloc *a = find_alloc(d); a && d + bytes <= a->base + a->size) set_written(*a, d, d + bytes);
    } else std::memset(dst, 0, bytes);
    b.ops.push_back(op);
    if (sync) merge(b.host, s->vc);
    return hipSuccess;
}

}  // namespace

const char *kind_name(int k)
{
    static const char *names[V_KINDS] = {"double-free", "out-of-bounds", "unwritten-read", "hazard", "leak", "dead-handle",
                                         "block-overlap", "check", "unmatched", "group-open", "size-mismatch", "comm-init"};
    return k >= 0 && k < V_KINDS ? names[k] : "?";
}
void violation(int kind, const std::string &what)
{
    Books &b = B();
    ++b.viol[kind];
    if (b.log.size() < 200) b.log.push_back(std::string(kind_name(kind)) + ": " + what);
}
uint64_t violations(int kind) { return B().viol[kind]; }
uint64_t violations_total()
{
    uint64_t n = 0;
    for (uint64_t v : B().viol) n += v;
    return n;
}
const std::vector<std::string> &violation_log() { return B().log; }
void expect_violations(int kind, uint64_t n, const std::string &why)
{
    Books &b = B();
    if (b.viol[kind] != n) {
        violation(V_CHECK, why + ": expected " + std::to_string(n) + " x " + kind_name(kind) + ", the books hold " + std::to_string(b.viol[kind]));
        return;
    }
    b.viol[kind] = 0;
    const std::string prefix = std::string(kind_name(kind)) + ": ";
    for (size_t i = 0; i < b.log.size();)
        if (b.log[i].compare(0, prefix.size(), prefix) == 0) b.log.erase(b.log.begin() + (std::ptrdiff_t)i);
        else ++i;
}

void reset()
{
    if (g) {
        for (auto &p : g->pinned) std::free(p.first);
        delete g;
    }
    g = new Books;
    for (int d = 0; d < N_DEV; ++d) {
        Stream s;
        s.id = d; s.dev = d;
        g->streams.push_back(s);
    }
    rccl_reset();
}

void arm(int64_t k, hipError_t error)
{
    Books &b = B();
    b.armed_k = k; b.armed_err = error; b.fired = false; b.fired_name.clear(); b.n_calls = 0;
}
void disarm() { B().armed_k = -1; }
bool fired() { return B().fired; }
const std::string &fired_name() { return B().fired_name; }
hipError_t fired_error() { return B().fired_err; }
uint64_t injectable_calls() { return B().n_calls; }

void declare(const char *name, FnClass cls)
{
    auto it = g_cov.find(name);
    if (it == g_cov.end()) g_cov[name] = Coverage{name, cls, 0, 0};
}
// Every injectable entry point this file defines: the runtime's half of the set the coverage condition is held to (the
// launchers' half: declare_launchers, fake_kernels.cpp).  enter() refuses a name that is in neither list, so the lists cannot
// fall behind the code.
void declare_runtime()
{
    for (const char *n : {"hipGetDeviceCount", "hipGetDevice", "hipSetDevice", "hipGetDeviceProperties", "hipMemGetInfo", "hipDeviceCanAccessPeer",
                          "hipDeviceEnablePeerAccess", "hipDeviceSynchronize", "hipMemcpy", "hipMemcpyAsync", "hipMemcpyPeerAsync",
                          "hipStreamSynchronize", "hipStreamWaitEvent", "hipStreamIsCapturing", "hipEventRecord", "hipEventSynchronize",
                          "hipEventElapsedTime"})
        declare(n, FN_OTHER);
    for (const char *n : {"hipMalloc", "hipHostMalloc", "hipStreamCreateWithFlags", "hipEventCreate", "hipEventCreateWithFlags"}) declare(n, FN_ALLOC);
    for (const char *n : {"hipFree", "hipHostFree", "hipStreamDestroy", "hipEventDestroy"}) declare(n, FN_RELEASE);
}
hipError_t enter(const char *name, FnClass cls)
{
    Books &b = B();
    if (!g_cov.count(name)) {
        violation(V_CHECK, std::string(name) + " is an injectable call site that no list declares (declare_runtime / declare_launchers)");
        declare(name, cls);
    }
    Coverage &c = g_cov[name];
    ++c.calls;
    const uint64_t idx = b.n_calls++;
    if (b.armed_k >= 0 && !b.fired && (int64_t)idx == b.armed_k) {
        b.fired = true; b.fired_name = name;
        b.fired_err = b.armed_err != hipSuccess ? b.armed_err
                      : cls == FN_ALLOC         ? hipErrorOutOfMemory
                      : cls == FN_LAUNCH        ? hipErrorLaunchFailure
                                                : hipErrorInvalidValue;
        ++c.failed;
        return err(b.fired_err);
    }
    return hipSuccess;
}
std::vector<Coverage> coverage()
{
    std::vector<Coverage> v;
    for (auto &kv : g_cov) v.push_back(kv.second);
    return v;
}
const std::vector<std::string> &not_injectable()
{
    static const std::vector<std::string> v = {"hipGetLastError", "hipGetErrorName", "hipGetErrorString"};
    return v;
}

void script_elapsed_ms(const std::vector<float> &values, float then)
{
    Books &b = B();
    b.elapsed = values; b.elapsed_next = 0; b.elapsed_then = then;
}
void set_capturing(hipStream_t s, bool on)
{
    if (Stream *p = stream(s, "set_capturing")) p->capturing = on;
}
void mark_written(const void *p, uint64_t bytes)
{
    const uint64_t lo = reinterpret_cast<uint64_t>(p);
    if (Alloc *a = find_alloc(lo)) set_written(*a, lo, std::min(lo + bytes, a->base + a->size));
}

Live live()
{
    Books &b = B();
    Live l{0, 0, 0, 0, 0};
    for (auto &kv : b.allocs)
        if (kv.second.live && !kv.second.orphan) { ++l.allocs; l.alloc_bytes += kv.second.size; }
    for (auto &p : b.pinned) l.pinned += !p.second;
    for (const Stream &s : b.streams) l.streams += s.id >= N_DEV && s.live && !s.orphan;
    for (const Event &e : b.events) l.events += e.live && !e.orphan;
    return l;
}
uint64_t orphans()
{
    Books &b = B();
    uint64_t n = 0;
    for (auto &kv : b.allocs) n += kv.second.live && kv.second.orphan;
    for (auto &p : b.pinned) n += p.second;
    for (const Stream &s : b.streams) n += s.live && s.orphan;
    for (const Event &e : b.events) n += e.live && e.orphan;
    return n;
}
Counters counters() { return B().cnt; }
void audit_leaks()
{
    Books &b = B();
    for (auto &kv : b.allocs)
        if (kv.second.live && !kv.second.orphan) violation(V_LEAK, "allocation of " + std::to_string(kv.second.size) + " bytes is still live");
    for (auto &p : b.pinned)
        if (!p.second) violation(V_LEAK, "a pinned host block is still live");
    for (const Stream &s : b.streams)
        if (s.id >= N_DEV && s.live && !s.orphan) violation(V_LEAK, "stream " + std::to_string(s.id) + " is still live");
    for (size_t i = 0; i < b.events.size(); ++i)
        if (b.events[i].live && !b.events[i].orphan) violation(V_LEAK, "event " + std::to_string(i) + " is still live");
    rccl_audit_leaks();
}

// ---- launches ----
namespace {

// The bytes a region covers, as few ranges as its shape allows: a dimension whose stride is the contiguous length so far
// extends that length (adjacent tiles of a row, adjacent rows of a matrix, adjacent transforms of a batch); what is left is
// enumerated.  `disjoint`: a dimension that steps by less than the length makes two blocks touch the same bytes.
bool fold(const Region &r, std::vector<Range> &out, bool *disjoint)
{
    uint64_t len = r.len;
    std::vector<Dim> dims;
    for (const Dim &d : r.dims)
        if (d.count == 0) return true;  // nothing at all
        else if (d.count > 1) dims.push_back(d);
    if (!len) return true;
    while (!dims.empty()) {  // the dimension with the smallest stride folds first, or nothing does
        size_t m = 0;
        for (size_t i = 1; i < dims.size(); ++i)
            if (dims[i].stride < dims[m].stride) m = i;
        if (dims[m].stride > len) break;
        if (dims[m].stride < len) *disjoint = false;
        len = dims[m].stride * (dims[m].count - 1) + len;
        dims.erase(dims.begin() + (std::ptrdiff_t)m);
    }
    uint64_t total = 1;
    for (const Dim &d : dims) {
        total *= d.count;
        if (total > (1u << 16)) return false;
    }
    const uint64_t base = reinterpret_cast<uint64_t>(r.base);
    std::vector<uint64_t> idx(dims.size(), 0);
    for (uint64_t n = 0; n < total; ++n) {
        uint64_t off = 0;
        for (size_t i = 0; i < dims.size(); ++i) off += idx[i] * dims[i].stride;
        out.push_back({base + off, base + off + len});
        for (size_t i = 0; i < dims.size(); ++i) {
            if (++idx[i] < dims[i].count) break;
            idx[i] = 0;
        }
    }
    return true;
}

}  // namespace

hipError_t launch(const char *name, hipStream_t st, const std::vector<Region> &reads, const std::vector<Region> &writes)
{
    if (hipError_t e = enter(name, FN_LAUNCH)) return e;
    Books &b = B();
    Stream *s = stream(st, name);
    if (!s) return err(hipErrorInvalidHandle);
    if (s->dev != b.current) violation(V_CHECK, std::string(name) + ": launched on a stream of a device that is not current");
    Op op{name, st, s->id, begin_op(*s), {}, {}, true};
    std::vector<Range> rd, wr;
    bool disjoint = true, unused = true;
    for (const Region &r : reads)
        if (!fold(r, rd, &unused)) violation(V_CHECK, std::string(name) + ": a read region does not fold to 2^16 ranges");
    for (const Region &r : writes)
        if (!fold(r, wr, &disjoint)) violation(V_CHECK, std::string(name) + ": a write region does not fold to 2^16 ranges");
    if (!disjoint) violation(V_BLOCK_OVERLAP, std::string(name) + ": two workgroups write the same bytes");
    for (const Range &r : rd) touch(op, r.lo, r.hi, false, *s, op.tick);
    for (const Range &r : wr) touch(op, r.lo, r.hi, true, *s, op.tick);
    for (const Range &r : op.writes)
        if (Alloc *a = find_alloc(r.lo)) set_written(*a, r.lo, r.hi);
    b.ops.push_back(op);
    return hipSuccess;
}
hipError_t setup(const char *name) { return enter(name, FN_OTHER); }
const std::vector<Op> &ops() { return B().ops; }
bool locate(uint64_t addr, uint64_t *base, uint64_t *size)
{
    Alloc *a = find_alloc(addr);
    if (!a) return false;
    *base = a->base; *size = a->size;
    return true;
}
void note_grid(uint64_t blocks) { B().grid = blocks; }
uint64_t last_grid() { return B().grid; }
int current_device() { return B().current; }

bool post(const char *who, hipStream_t st, Post *out)
{
    Books &b = B();
    Stream *s = stream(st, who);
    if (!s) return false;
    if (s->dev != b.current) violation(V_CHECK, std::string(who) + ": posted on a stream of a device that is not current");
    out->tick = begin_op(*s);
    out->sid = s->id; out->dev = b.current; out->clock = s->vc;
    return true;
}

void transfer(const std::string &name, const Post &src, uint64_t src_addr, const Post &dst, uint64_t dst_addr, uint64_t bytes)
{
    Books &b = B();
    VC when = src.clock;
    merge(when, dst.clock);
    // the two sides as the streams they were posted on, at their posted ticks, both knowing what either stream knew
    Stream from, to;
    from.id = src.sid; from.dev = src.dev; from.vc = when;
    to.id = dst.sid; to.dev = dst.dev; to.vc = when;
    Op op{name, nullptr, dst.sid, dst.tick, {}, {}, false};
    touch(op, src_addr, src_addr + bytes, false, from, src.tick);
    touch(op, dst_addr, dst_addr + bytes, true, to, dst.tick);
    for (const Range &r : op.writes)
        if (Alloc *a = find_alloc(r.lo)) set_written(*a, r.lo, r.hi);
    b.ops.push_back(op);
    // everything later on either stream is behind the transfer
    merge(b.streams[(size_t)src.sid].vc, when);
    merge(b.streams[(size_t)dst.sid].vc, when);
}

bool all_before_marker(size_t first, hipStream_t caller, std::string *which)
{
    Books &b = B();
    Stream *s = stream(caller, "marker");
    if (!s) return false;
    VC vc = s->vc;
    merge(vc, b.host);
    for (size_t i = first; i < b.ops.size(); ++i)
        if (b.ops[i].sid != s->id && at(vc, (size_t)b.ops[i].sid) < b.ops[i].tick) {
            if (which) *which = b.ops[i].name + " on stream " + std::to_string(b.ops[i].sid);
            return false;
        }
    return true;
}

}  // namespace sim

using namespace sim;

// ===================================================== the runtime =====================================================
#define ENTER(cls)                                          \
    do {                                                    \
        if (hipError_t e_ = sim::enter(__func__, cls)) return e_; \
    } while (0)

extern "C" {

hipError_t hipGetLastError(void)
{
    Books &b = B();
    const hipError_t e = b.sticky;
    b.sticky = hipSuccess;
    return e;
}
const char *hipGetErrorName(hipError_t e)
{
    switch (e) {
        case hipSuccess: return "hipSuccess";
        case hipErrorInvalidValue: return "hipErrorInvalidValue";
        case hipErrorOutOfMemory: return "hipErrorOutOfMemory";
        case hipErrorLaunchFailure: return "hipErrorLaunchFailure";
        case hipErrorInvalidHandle: return "hipErrorInvalidHandle";
        case hipErrorInvalidDevice: return "hipErrorInvalidDevice";
        case hipErrorNotReady: return "hipErrorNotReady";
        case hipErrorPeerAccessAlreadyEnabled: return "hipErrorPeerAccessAlreadyEnabled";
        default: return "hipErrorUnknown";
    }
}
const char *hipGetErrorString(hipError_t e)
{
    switch (e) {
        case hipSuccess: return "no error";
        case hipErrorInvalidValue: return "invalid argument";
        case hipErrorOutOfMemory: return "out of memory";
        case hipErrorLaunchFailure: return "unspecified launch failure";
        case hipErrorInvalidHandle: return "invalid resource handle";
        case hipErrorInvalidDevice: return "invalid device ordinal";
        default: return "unknown error";
    }
}

// ---- devices ----
hipError_t hipGetDeviceCount(int *count)
{
    ENTER(FN_OTHER);
    *count = N_DEV;
    return hipSuccess;
}
hipError_t hipGetDevice(int *dev)
{
    ENTER(FN_OTHER);
    *dev = B().current;
    return hipSuccess;
}
hipError_t hipSetDevice(int dev)
{
    ENTER(FN_OTHER);
    if (dev < 0 || dev >= N_DEV) return err(hipErrorInvalidDevice);
    B().current = dev;
    return hipSuccess;
}
hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int dev)
{
    // (the header renames this function with a version suffix: the books keep the API's name)
    if (hipError_t e_ = sim::enter("hipGetDeviceProperties", FN_OTHER)) return e_;
    if (dev < 0 || dev >= N_DEV) return err(hipErrorInvalidDevice);
    std::memset(prop, 0, sizeof *prop);
    std::snprintf(prop->name, sizeof prop->name, "simulated MI355X #%d", dev);
    std::snprintf(prop->gcnArchName, sizeof prop->gcnArchName, "gfx950:sramecc+:xnack-");
    prop->totalGlobalMem = HBM_BYTES;
    prop->multiProcessorCount = 256;
    prop->warpSize = 64;
    prop->maxThreadsPerBlock = 1024;
    prop->sharedMemPerBlock = 64 << 10;
    prop->maxSharedMemoryPerMultiProcessor = 160 << 10;
    prop->l2CacheSize = 4 << 20;
    prop->major = 9; prop->minor = 5;
    return hipSuccess;
}
hipError_t hipMemGetInfo(size_t *free_bytes, size_t *total)
{
    ENTER(FN_OTHER);
    Books &b = B();
    *total = HBM_BYTES;
    *free_bytes = HBM_BYTES - b.live_bytes[b.current];
    return hipSuccess;
}
hipError_t hipDeviceCanAccessPeer(int *can, int dev, int peer)
{
    ENTER(FN_OTHER);
    if (dev < 0 || dev >= N_DEV || peer < 0 || peer >= N_DEV) return err(hipErrorInvalidDevice);
    *can = dev != peer;
    return hipSuccess;
}
hipError_t hipDeviceEnablePeerAccess(int peer, unsigned int flags)
{
    ENTER(FN_OTHER);
    Books &b = B();
    if (peer < 0 || peer >= N_DEV || peer == b.current || flags) return err(hipErrorInvalidDevice);
    if (b.peer[b.current][peer]) return err(hipErrorPeerAccessAlreadyEnabled);
    b.peer[b.current][peer] = true;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void)
{
    ENTER(FN_OTHER);
    Books &b = B();
    for (const Stream &s : b.streams)  // the work of a destroyed stream is waited for like any other
        if (s.dev == b.current) {
            if (s.live && s.capturing) return err(hipErrorStreamCaptureUnsupported);  // illegal while a stream of the device captures
            merge(b.host, s.vc);
        }
    return hipSuccess;
}

// ---- memory ----
hipError_t hipMalloc(void **p, size_t bytes)
{
    ENTER(FN_ALLOC);
    Books &b = B();
    *p = nullptr;
    if (!bytes) return hipSuccess;
    const int d = b.current;
    if (b.live_bytes[d] + bytes > HBM_BYTES) return err(hipErrorOutOfMemory);
    Alloc a;
    a.dev = d; a.base = dev_base(d) + b.bump[d]; a.size = bytes;
    b.bump[d] += (bytes + GUARD + ALIGN - 1) / ALIGN * ALIGN;
    b.live_bytes[d] += bytes;
    b.allocs[a.base] = a;
    ++b.cnt.mallocs;
    *p = reinterpret_cast<void *>(a.base);
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    Books &b = B();
    const hipError_t inj = sim::enter(__func__, FN_RELEASE);
    if (!p) return inj;
    auto it = b.allocs.find(reinterpret_cast<uint64_t>(p));
    if (it == b.allocs.end() || !it->second.live) {
        violation(V_DOUBLE_FREE, it == b.allocs.end() ? "hipFree of a pointer no hipMalloc returned" : "hipFree of memory already freed");
        return err(hipErrorInvalidValue);
    }
    if (inj) { it->second.orphan = true; return inj; }  // nothing released: the audit lists it apart
    for (const Stream &s : b.streams)  // hipFree synchronises the device
        if (s.dev == it->second.dev) merge(b.host, s.vc);
    it->second.live = false;
    it->second.hist.clear();
    it->second.written.clear();
    b.live_bytes[it->second.dev] -= it->second.size;
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int)
{
    ENTER(FN_ALLOC);
    Books &b = B();
    *p = std::malloc(bytes ? bytes : 1);  // ordinary memory: AddressSanitizer guards it
    if (!*p) return err(hipErrorOutOfMemory);
    b.pinned[*p] = false;
    ++b.cnt.host_mallocs;
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    Books &b = B();
    const hipError_t inj = sim::enter(__func__, FN_RELEASE);
    if (!p) return inj;
    auto it = b.pinned.find(p);
    if (it == b.pinned.end()) {
        violation(V_DOUBLE_FREE, "hipHostFree of a pointer that is not a live pinned block");
        return err(hipErrorInvalidValue);
    }
    if (inj) { it->second = true; return inj; }
    std::free(p);
    b.pinned.erase(it);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    ENTER(FN_OTHER);
    const int d = B().current;
    return copy(__func__, dst, d, src, d, bytes, kind, nullptr, true);
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
    ENTER(FN_OTHER);
    const int d = B().current;
    return copy(__func__, dst, d, src, d, bytes, kind, st, false);
}
hipError_t hipMemcpyPeerAsync(void *dst, int dst_dev, const void *src, int src_dev, size_t bytes, hipStream_t st)
{
    ENTER(FN_OTHER);
    Books &b = B();
    if (dst_dev < 0 || dst_dev >= N_DEV || src_dev < 0 || src_dev >= N_DEV) return err(hipErrorInvalidDevice);
    if (dst_dev != src_dev && !(b.peer[dst_dev][src_dev] && b.peer[src_dev][dst_dev]))
        violation(V_CHECK, "hipMemcpyPeerAsync between devices whose peer access was never enabled");
    return copy(__func__, dst, dst_dev, src, src_dev, bytes, hipMemcpyDeviceToDevice, st, false);
}

// ---- streams ----
hipError_t hipStreamCreateWithFlags(hipStream_t *out, unsigned int flags)
{
    ENTER(FN_ALLOC);
    Books &b = B();
    Stream s;
    s.id = (int)b.streams.size(); s.dev = b.current; s.flags = flags;
    b.streams.push_back(s);
    b.stream_of[stream_handle(s.id)] = s.id;
    ++b.cnt.streams_created;
    *out = stream_handle(s.id);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t h)
{
    const hipError_t inj = sim::enter(__func__, FN_RELEASE);
    if (!h) { violation(V_DEAD_HANDLE, "hipStreamDestroy of the null stream"); return err(hipErrorInvalidHandle); }
    Stream *s = stream(h, __func__);
    if (!s) return err(hipErrorInvalidHandle);
    if (inj) { s->orphan = true; return inj; }
    s->live = false;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t h)
{
    ENTER(FN_OTHER);
    Stream *s = stream(h, __func__);
    if (!s) return err(hipErrorInvalidHandle);
    merge(B().host, s->vc);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t h, hipEvent_t ev, unsigned int)
{
    ENTER(FN_OTHER);
    Stream *s = stream(h, __func__);
    Event *e = event(ev, __func__);
    if (!s || !e) return err(hipErrorInvalidHandle);
    if (e->recorded) merge(s->vc, e->snap);  // an event never recorded is complete: the wait is a no-op
    return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t h, hipStreamCaptureStatus *status)
{
    ENTER(FN_OTHER);
    Stream *s = stream(h, __func__);
    if (!s) return err(hipErrorInvalidHandle);
    *status = s->capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}

// ---- events ----
static hipError_t new_event(hipEvent_t *out)
{
    Books &b = B();
    Event e;
    e.dev = b.current;
    b.events.push_back(e);
    const int id = (int)b.events.size() - 1;
    b.event_of[event_handle(id)] = id;
    ++b.cnt.events_created;
    *out = event_handle(id);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *out, unsigned int)
{
    ENTER(FN_ALLOC);
    return new_event(out);
}
hipError_t hipEventCreate(hipEvent_t *out)
{
    ENTER(FN_ALLOC);
    return new_event(out);
}
hipError_t hipEventDestroy(hipEvent_t ev)
{
    const hipError_t inj = sim::enter(__func__, FN_RELEASE);
    Event *e = event(ev, __func__);
    if (!e) return err(hipErrorInvalidHandle);
    if (inj) { e->orphan = true; return inj; }
    e->live = false;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t h)
{
    ENTER(FN_OTHER);
    Stream *s = stream(h, __func__);
    Event *e = event(ev, __func__);
    if (!s || !e) return err(hipErrorInvalidHandle);
    if (s->capturing) return hipSuccess;  // captured into the graph: nothing real is recorded
    (void)begin_op(*s);
    e->snap = s->vc;
    e->recorded = true;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev)
{
    ENTER(FN_OTHER);
    Event *e = event(ev, __func__);
    if (!e) return err(hipErrorInvalidHandle);
    if (e->recorded) merge(B().host, e->snap);
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop)
{
    ENTER(FN_OTHER);
    Books &b = B();
    Event *e0 = event(start, __func__), *e1 = event(stop, __func__);
    if (!e0 || !e1) return err(hipErrorInvalidHandle);
    if (!e0->recorded || !e1->recorded) return err(hipErrorInvalidHandle);
    *ms = b.elapsed_next < b.elapsed.size() ? b.elapsed[b.elapsed_next++] : b.elapsed_then;
    return hipSuccess;
}

}  // extern "C"
