// fake_hip.h -- what the three files of tools/host_sim share: the books of the simulated HIP runtime (fake_hip.cpp), the
// launch recorder the simulated launchers report to (fake_kernels.cpp) and the queries the scenarios ask (host_faults.cpp).
// Nothing here touches a device: device memory is address space only, streams and events are counted handles with logical
// clocks.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

namespace sim {

// ---- violations: every check of the fake reports one of these kinds; a clean run has none ----
enum Kind {
    V_DOUBLE_FREE,     // hipFree / hipHostFree of an unknown or dead pointer
    V_OUT_OF_BOUNDS,   // a copy or a launch range that does not lie inside one live allocation of the right device
    V_UNWRITTEN_READ,  // a copy from the device or a launch reads bytes nothing has written
    V_HAZARD,          // two accesses overlap, one writes, and the earlier does not happen-before the later
    V_LEAK,            // a live allocation, pinned block, stream or event at the audit
    V_DEAD_HANDLE,     // a stream or event that is unknown or destroyed is used or destroyed
    V_BLOCK_OVERLAP,   // two workgroups of one launch write the same bytes
    V_CHECK,           // a property the scenarios assert (status, error string, getters, launch counts ...)
    V_UNMATCHED,       // fake_rccl.cpp: a send or receive still pending when the collective is declared complete ("waits for ever")
    V_GROUP_OPEN,      // fake_rccl.cpp: an ncclGroupStart without its ncclGroupEnd when the library call has returned
    V_SIZE_MISMATCH,   // fake_rccl.cpp: a send met a receive of another byte count
    V_COMM_INIT,       // fake_rccl.cpp: a second rank on one device, a repeated rank, a world other than the id's first caller's
    V_KINDS
};
const char *kind_name(int kind);
void violation(int kind, const std::string &what);
uint64_t violations(int kind);  // since the last reset()
uint64_t violations_total();
const std::vector<std::string> &violation_log();
// A scenario that provokes a violation on purpose (a positive test of a check): exactly `n` of `kind` must be on the books; they are
// taken off (log lines too).  Anything else is a V_CHECK and the books stay.
void expect_violations(int kind, uint64_t n, const std::string &why);

// ---- life of the fake ----
void reset();  // fresh books: no allocation, stream or event, clocks at zero, nothing armed, sticky error cleared

// ---- injection: the k-th injectable call counted from arm() returns an error and does nothing else.  error == hipSuccess
// picks it by the class of the function that is hit: out-of-memory for allocations, a launch failure for launchers,
// invalid-value otherwise ----
void arm(int64_t k, hipError_t error = hipSuccess);
void disarm();
bool fired();                        // the armed call has happened
const std::string &fired_name();     // which function it was
hipError_t fired_error();
uint64_t injectable_calls();         // counted since reset() / arm()
// Called first by every injectable entry point, runtime function or launcher: counts the call; non-zero = fail with it.
enum FnClass { FN_ALLOC, FN_LAUNCH, FN_OTHER, FN_RELEASE };
hipError_t enter(const char *name, FnClass cls);
// coverage over the whole process (survives reset): calls seen and times each injectable function was the failing call
struct Coverage { std::string name; FnClass cls; uint64_t calls, failed; };
std::vector<Coverage> coverage();
// The expected set of the coverage condition: every injectable entry point of fake_hip.cpp (declare_runtime) and every launcher
// and setup of fake_kernels.cpp (declare_launchers), listed before anything runs so that a function no scenario reaches shows
// in the table with zero calls.  enter() reports a name that was never declared.
void declare(const char *name, FnClass cls);
void declare_runtime();
void declare_launchers();
const std::vector<std::string> &not_injectable();

// ---- knobs of the scenarios ----
void script_elapsed_ms(const std::vector<float> &values, float then);  // answers of hipEventElapsedTime, in order
void set_capturing(hipStream_t s, bool on);                            // hipStreamIsCapturing reports capture on s
void mark_written(const void *p, uint64_t bytes);                      // as an upload would

// ---- books ----
struct Live { uint64_t allocs, alloc_bytes, pinned, streams, events; };
Live live();                   // resources whose release failed by injection are not counted (they are listed by orphans())
uint64_t orphans();
struct Counters { uint64_t mallocs, host_mallocs, streams_created, events_created; };
Counters counters();           // since reset()
void audit_leaks();            // a V_LEAK per live resource

// ---- launches and copies: one record per operation that touches device memory ----
struct Dim { uint64_t count, stride; };                 // stride in bytes
struct Region { const void *base; uint64_t len; std::vector<Dim> dims; };  // `len` contiguous bytes at base + sum(i_d * stride_d)
struct Range { uint64_t lo, hi; };
struct Op {
    std::string name;
    hipStream_t stream;
    int sid;                         // the fake's stream id
    uint64_t tick;                   // position on that stream
    std::vector<Range> reads, writes;
    bool launch;
};
// A launcher's whole job: injectable call site, fold the regions to ranges, checks (a) bounds, (b) written, (c) hazards, mark
// the writes written, record.
hipError_t launch(const char *name, hipStream_t st, const std::vector<Region> &reads, const std::vector<Region> &writes);
hipError_t setup(const char *name);  // a kernel-family setup: injectable, touches nothing
const std::vector<Op> &ops();
// where a device address lies: false if in no allocation
bool locate(uint64_t addr, uint64_t *alloc_base, uint64_t *alloc_size);
// Would a marker recorded NOW on `caller` be ordered behind every operation ops()[first ..]?
bool all_before_marker(size_t first, hipStream_t caller, std::string *which);
// the grid of the last launch whose launcher reported one (the framed plans: compared with fwt_describe)
void note_grid(uint64_t blocks);
uint64_t last_grid();

// ---- what the simulated RCCL (fake_rccl.cpp) needs of the books ----
int current_device();
// A position reserved on stream `st` of the current device when a send or a receive is posted: the stream's tick and its clock.
// false (and a violation) for a dead handle; a stream of another device than the current one is a V_CHECK.
struct Post { int sid = -1, dev = -1; uint64_t tick = 0; std::vector<uint64_t> clock; };
bool post(const char *who, hipStream_t st, Post *out);
// A matched transfer.  Both ranges are checked against live allocations of the POSTING rank's device, the source must be
// written; the transfer is ordered behind everything earlier on both streams (the two posted clocks merged) and everything later
// on either stream is ordered behind it; hazards as for any operation; the destination is marked written.  One Op is recorded.
void transfer(const std::string &name, const Post &src, uint64_t src_addr, const Post &dst, uint64_t dst_addr, uint64_t bytes);
void rccl_reset();         // fake_rccl.cpp: fresh books, called by reset()
void rccl_audit_leaks();   // fake_rccl.cpp: a V_LEAK per live communicator, called by audit_leaks()

// ---- the simulated RCCL's books (fake_rccl.cpp, whose header comment has the rules) ----
void declare_rccl();                             // its seven injectable entry points, for the coverage condition
uint64_t rccl_calls();                           // calls of any entry point, over the whole process: proof that the fake answered
uint64_t rccl_live();                            // communicators registered and not destroyed
uint64_t rccl_pending();                         // sends and receives that wait for their partner
uint64_t rccl_complete(const std::string &what); // "every rank has made this call": a V_UNMATCHED per pending operation, then dropped
bool rccl_group_closed(const std::string &after);// a library call has returned: V_GROUP_OPEN (and the group is dropped) if one is open
struct RcclRecord { int src_rank; uint64_t src, bytes; int dst_rank; uint64_t dst; };
const std::vector<RcclRecord> &rccl_records();   // every matched transfer since reset() / rccl_clear_records()
void rccl_clear_records();

}  // namespace sim
