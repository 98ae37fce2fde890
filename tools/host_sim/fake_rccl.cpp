// fake_rccl.cpp -- a simulated RCCL for fft_wgpu_amd/csrc/comm.cpp: the CONTRACT of the eight entry points comm.cpp resolves,
// none of RCCL's code.  comm.cpp loads RCCL with dlopen("librccl.so.1"), so this file is compiled twice:
//   -DFAKE_RCCL_SHARED   a small shared object named librccl.so.1 (tests/test_host_faults.py builds it into its temporary directory
//                        and puts that directory into the child's LD_LIBRARY_PATH).  It defines the eight entry points against the
//                        installed <rccl/rccl.h> and does nothing but forward to the fake_rccl_* functions below, which it finds in
//                        the program (linked with -rdynamic).  It carries no sanitizer: it holds no logic to guard.
//                        -DFAKE_RCCL_NO_RECV leaves ncclRecv out: the stub of the "symbol missing" run.
//   (no macro)           the books and the rules, linked into the program beside fake_hip.cpp under AddressSanitizer + UBSan.
// Ranks are driven one after another from ONE thread, so nothing here blocks: an operation whose partner has not been posted yet
// waits in a queue, and the match completes when the second side posts.  The scenarios therefore finish each collective on every
// rank before they enqueue dependent work (sim::rccl_complete), as the deferred match requires.
//
// The rules, and what each rests on (line numbers of rccl/rccl.h as installed with ROCm, doc = the NCCL user guide, "Group Calls"
// and "Point-to-point communication"):
//   ncclGetUniqueId   fills the 128 bytes (rccl.h:40, 187) with a serial number.  Every entry point counts its call in
//                     sim::rccl_calls(): the scenarios refuse to run unless that counter moves, i.e. unless THIS library answered.
//   ncclCommInitRank  rccl.h:209-220: "Rank must be between 0 and nranks-1 and unique within a communicator clique.  Each rank is
//                     associated to a CUDA device, which has to be set before calling ncclCommInitRank."  Registers (id, world, rank,
//                     current device) and returns at once (the real call waits for the other ranks; one thread cannot).  V_COMM_INIT:
//                     a rank already registered under the id, a second rank of the id on one device (doc: one device used as several ranks of
//                     one communicator is not supported and may hang; RCCL answers ncclInvalidUsage), a world other than the
//                     one the id's first caller gave.
//   ncclGroupStart /  rccl.h:919-933: "All calls to RCCL until ncclGroupEnd will be fused into a single RCCL operation.  Nothing
//   ncclGroupEnd      will be started on the HIP stream until ncclGroupEnd."  So the operations of a group take their place on their
//                     streams at the outermost ncclGroupEnd, in call order.  V_GROUP_OPEN (sim::rccl_group_closed, asked by the
//                     scenarios when a library call has returned): a group still open.  An ncclGroupEnd that fails by injection
//                     still closes the group and discards its operations, and so does the ncclGroupEnd of a group in which a send
//                     or a receive failed (it answers ncclInternalError); one without a group is a V_CHECK.
//   ncclSend /        rccl.h:685-723: "Rank peer needs to call ncclRecv with the same datatype and the same count as this rank ...
//   ncclRecv          If multiple ncclSend and ncclRecv operations need to progress concurrently to complete, they must be fused
//                     within a ncclGroupStart / ncclGroupEnd section."  Outside a group an operation is legal only alone; comm.cpp
//                     never does that, so it is reported (V_CHECK) and handled as a group of one.  Operations are matched in
//                     posting order per (id, sending rank, receiving rank) (doc: point-to-point operations between two ranks match
//                     in the order they are issued).  On a match: equal byte counts or V_SIZE_MISMATCH (nothing moves); both ranges
//                     inside live allocations of the POSTING rank's device (V_OUT_OF_BOUNDS), the source written
//                     (V_UNWRITTEN_READ), ordered behind everything earlier on both streams and before everything later, hazards
//                     as for any operation (sim::transfer); the destination is marked written; a record (source rank, address,
//                     bytes, destination rank, address) is kept (sim::rccl_records).
//                     A send to the own rank is a local copy when its receive is in the same group (doc: a rank may send to itself if the
//                     matching receive is issued in the same group); without it, and likewise a receive from self without its
//                     send, V_UNMATCHED at ncclGroupEnd.  A peer outside [0, world) is ncclInvalidArgument and a V_CHECK (comm.cpp
//                     refuses such a rank before it gets here).
//   ncclCommDestroy   drops what the communicator's rank still has pending (a failed collective leaves the peers' operations behind:
//                     include/fft_wgpu_amd.h, "Errors in a collective are fatal for the COMMUNICATOR") and frees the registration.
//                     A communicator alive at the audit is a V_LEAK.
//   sim::rccl_complete(what)   the scenario's statement that a collective has been called on every rank: every operation still
//                     pending is a V_UNMATCHED -- on a GPU, a stream that waits for ever.
//   ncclGetErrorString is the only entry point that cannot fail by injection; the other seven enter sim::enter like the runtime.
#include <rccl/rccl.h>

#include <cstdint>

extern "C" {
ncclResult_t fake_rccl_get_unique_id(ncclUniqueId *id);
ncclResult_t fake_rccl_comm_init_rank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank);
ncclResult_t fake_rccl_comm_destroy(ncclComm_t comm);
ncclResult_t fake_rccl_group_start(void);
ncclResult_t fake_rccl_group_end(void);
ncclResult_t fake_rccl_send(const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream);
ncclResult_t fake_rccl_recv(void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream);
const char *fake_rccl_error_string(ncclResult_t e);
}

#ifdef FAKE_RCCL_SHARED
// ======================================= librccl.so.1: forwarding only =======================================
extern "C" {
int fake_rccl_marker = 1;  // how the program tells this object from an installed RCCL (dlsym)
ncclResult_t ncclGetUniqueId(ncclUniqueId *id) { return fake_rccl_get_unique_id(id); }
ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank) { return fake_rccl_comm_init_rank(comm, nranks, id, rank); }
ncclResult_t ncclCommDestroy(ncclComm_t comm) { return fake_rccl_comm_destroy(comm); }
ncclResult_t ncclGroupStart() { return fake_rccl_group_start(); }
ncclResult_t ncclGroupEnd() { return fake_rccl_group_end(); }
ncclResult_t ncclSend(const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    return fake_rccl_send(buf, count, type, peer, comm, stream);
}
#ifndef FAKE_RCCL_NO_RECV
ncclResult_t ncclRecv(void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    return fake_rccl_recv(buf, count, type, peer, comm, stream);
}
#endif
const char *ncclGetErrorString(ncclResult_t e) { return fake_rccl_error_string(e); }
}
#else
// ======================================= the books and the rules (in the program) =======================================
#include <cstring>
#include <deque>
#include <map>
#include <tuple>

#include "fake_hip.h"

namespace {

struct CommRec { uint64_t id; int world, rank, dev; };
struct Pending {  // one side of a transfer that has its place on a stream and waits for the other side
    CommRec *comm;
    bool send;
    int peer;
    uint64_t addr, bytes;
    sim::Post at;
};
struct Queued { CommRec *comm; bool send; int peer; uint64_t addr, bytes; hipStream_t stream; };  // inside an open group

struct Books {
    uint64_t next_id = 1;
    std::map<uint64_t, int> world_of;                    // id -> the world its first caller gave
    std::map<CommRec *, bool> comms;                     // every live registration
    int depth = 0;
    bool group_failed = false;                           // a send or receive of the open group failed
    std::vector<Queued> group;
    // (id, sending rank, receiving rank) -> sends posted, receives posted: one of the two is empty at any time
    std::map<std::tuple<uint64_t, int, int>, std::pair<std::deque<Pending>, std::deque<Pending>>> wait;
    std::vector<sim::RcclRecord> records;
};
Books *g = nullptr;
uint64_t g_calls = 0;  // whole process
Books &B()
{
    if (!g) g = new Books;
    return *g;
}

std::string rank_name(const CommRec *c) { return "rank " + std::to_string(c->rank) + " of " + std::to_string(c->world); }

// a failing call by injection: RCCL reports what went wrong beneath it as one of its own codes
ncclResult_t counted(const char *name, sim::FnClass cls)
{
    ++g_calls;
    const hipError_t e = sim::enter(name, cls);
    return e == hipSuccess ? ncclSuccess : e == hipErrorOutOfMemory ? ncclSystemError : ncclUnhandledCudaError;
}

CommRec *live_comm(ncclComm_t h, const char *who)
{
    CommRec *c = reinterpret_cast<CommRec *>(h);
    if (!c || !B().comms.count(c)) {
        sim::violation(sim::V_DEAD_HANDLE, std::string(who) + ": unknown or destroyed communicator");
        return nullptr;
    }
    return c;
}

void match(const Pending &s, const Pending &r)
{
    const std::string name = "transfer " + rank_name(s.comm) + " -> rank " + std::to_string(r.comm->rank);
    if (s.bytes != r.bytes) {
        sim::violation(sim::V_SIZE_MISMATCH, name + ": " + std::to_string(s.bytes) + " bytes sent, " + std::to_string(r.bytes) + " expected");
        return;
    }
    if (s.bytes) sim::transfer(name, s.at, s.addr, r.at, r.addr, s.bytes);
    B().records.push_back({s.comm->rank, s.addr, s.bytes, r.comm->rank, r.addr});
}

// the outermost ncclGroupEnd: every operation takes its place on its stream, then meets its partner or waits
void submit()
{
    Books &b = B();
    std::vector<Queued> ops;
    ops.swap(b.group);
    std::vector<bool> used(ops.size(), false);
    for (size_t i = 0; i < ops.size(); ++i) {
        if (used[i]) continue;
        const Queued &q = ops[i];
        Pending p{q.comm, q.send, q.peer, q.addr, q.bytes, {}};
        if (!sim::post(q.send ? "ncclSend" : "ncclRecv", q.stream, &p.at)) continue;
        if (q.peer == q.comm->rank) {  // a local copy: its partner is the first unused opposite self operation of this group
            size_t j = i + 1;
            while (j < ops.size() && (used[j] || ops[j].comm != q.comm || ops[j].peer != q.peer || ops[j].send == q.send)) ++j;
            if (j == ops.size()) {
                sim::violation(sim::V_UNMATCHED, rank_name(q.comm) + (q.send ? ": a send to" : ": a receive from") +
                                                     " the rank itself without its partner in the same group");
                continue;
            }
            used[j] = true;
            Pending o{ops[j].comm, ops[j].send, ops[j].peer, ops[j].addr, ops[j].bytes, {}};
            if (!sim::post(o.send ? "ncclSend" : "ncclRecv", ops[j].stream, &o.at)) continue;
            match(p.send ? p : o, p.send ? o : p);
            continue;
        }
        auto &w = b.wait[std::make_tuple(q.comm->id, q.send ? q.comm->rank : q.peer, q.send ? q.peer : q.comm->rank)];
        std::deque<Pending> &mine = q.send ? w.first : w.second, &theirs = q.send ? w.second : w.first;
        if (theirs.empty()) { mine.push_back(p); continue; }
        const Pending o = theirs.front();
        theirs.pop_front();
        match(p.send ? p : o, p.send ? o : p);
    }
}

ncclResult_t operation(const char *name, bool send, const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    Books &b = B();
    if (ncclResult_t e = counted(name, sim::FN_OTHER)) {
        b.group_failed = b.depth > 0;
        return e;
    }
    CommRec *c = live_comm(comm, name);
    if (!c) return ncclInvalidArgument;
    if (peer < 0 || peer >= c->world) {
        sim::violation(sim::V_CHECK, std::string(name) + ": peer " + std::to_string(peer) + " is outside the world of " + std::to_string(c->world));
        return ncclInvalidArgument;
    }
    if (type != ncclInt8 && type != ncclUint8) sim::violation(sim::V_CHECK, std::string(name) + ": comm.cpp moves bytes, this is another datatype");
    if (sim::current_device() != c->dev)
        sim::violation(sim::V_CHECK, std::string(name) + ": the communicator's device is not the current one");
    b.group.push_back({c, send, peer, reinterpret_cast<uint64_t>(buf), (uint64_t)count, stream});
    if (b.depth == 0) {
        sim::violation(sim::V_CHECK, std::string(name) + " outside a group: legal alone, but comm.cpp always groups");
        submit();
    }
    return ncclSuccess;
}

}  // namespace

namespace sim {

void declare_rccl()
{
    for (const char *n : {"ncclGetUniqueId", "ncclGroupStart", "ncclGroupEnd", "ncclSend", "ncclRecv"}) declare(n, FN_OTHER);
    declare("ncclCommInitRank", FN_ALLOC);
    declare("ncclCommDestroy", FN_RELEASE);
}
uint64_t rccl_calls() { return g_calls; }
void rccl_reset()
{
    if (g) {
        for (auto &kv : g->comms) delete kv.first;
        delete g;
    }
    g = new Books;
}
void rccl_audit_leaks()
{
    for (auto &kv : B().comms) violation(V_LEAK, "communicator of " + rank_name(kv.first) + " is still live");
}
uint64_t rccl_live() { return B().comms.size(); }
uint64_t rccl_pending()
{
    uint64_t n = 0;
    for (auto &kv : B().wait) n += kv.second.first.size() + kv.second.second.size();
    return n;
}
uint64_t rccl_complete(const std::string &what)
{
    uint64_t n = 0;
    for (auto &kv : B().wait) {
        for (int side = 0; side < 2; ++side)
            for (const Pending &p : side ? kv.second.second : kv.second.first) {
                violation(V_UNMATCHED, what + ": " + rank_name(p.comm) + (p.send ? " sends " : " receives ") + std::to_string(p.bytes) + " bytes " +
                                           (p.send ? "to" : "from") + " rank " + std::to_string(p.peer) + " and nobody answers: its stream waits for ever");
                ++n;
            }
        kv.second.first.clear();
        kv.second.second.clear();
    }
    return n;
}
bool rccl_group_closed(const std::string &after)
{
    Books &b = B();
    if (b.depth == 0) return true;
    violation(V_GROUP_OPEN, after + " returned with an ncclGroupStart that has no ncclGroupEnd");
    b.depth = 0;
    b.group.clear();
    b.group_failed = false;
    return false;
}
const std::vector<RcclRecord> &rccl_records() { return B().records; }
void rccl_clear_records() { B().records.clear(); }

}  // namespace sim

extern "C" {

ncclResult_t fake_rccl_get_unique_id(ncclUniqueId *id)
{
    if (ncclResult_t e = counted("ncclGetUniqueId", sim::FN_OTHER)) return e;
    std::memset(id, 0, sizeof *id);
    const uint64_t n = B().next_id++;
    std::memcpy(id->internal, &n, sizeof n);
    return ncclSuccess;
}

ncclResult_t fake_rccl_comm_init_rank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank)
{
    if (ncclResult_t e = counted("ncclCommInitRank", sim::FN_ALLOC)) return e;
    Books &b = B();
    uint64_t key = 0;
    std::memcpy(&key, id.internal, sizeof key);
    const std::string who = "ncclCommInitRank(rank " + std::to_string(rank) + " of " + std::to_string(nranks) + ")";
    if (key == 0 || key >= b.next_id) sim::violation(sim::V_CHECK, who + ": an id that ncclGetUniqueId never gave");
    if (rank < 0 || rank >= nranks) { sim::violation(sim::V_CHECK, who + ": rank outside the world"); return ncclInvalidArgument; }
    if (!b.world_of.count(key)) b.world_of[key] = nranks;
    ncclResult_t bad = ncclSuccess;
    if (b.world_of[key] != nranks) {
        sim::violation(sim::V_COMM_INIT, who + ": the id's first caller said a world of " + std::to_string(b.world_of[key]));
        bad = ncclInvalidArgument;
    }
    for (auto &kv : b.comms)
        if (kv.first->id == key && kv.first->rank == rank) {
            sim::violation(sim::V_COMM_INIT, who + ": the rank is registered already");
            bad = ncclInvalidArgument;
        } else if (kv.first->id == key && kv.first->dev == sim::current_device()) {
            sim::violation(sim::V_COMM_INIT, who + ": device " + std::to_string(kv.first->dev) + " holds rank " + std::to_string(kv.first->rank) + " already");
            bad = ncclInvalidUsage;
        }
    if (bad != ncclSuccess) return bad;
    CommRec *c = new CommRec{key, nranks, rank, sim::current_device()};
    b.comms[c] = true;
    *comm = reinterpret_cast<ncclComm_t>(c);
    return ncclSuccess;
}

ncclResult_t fake_rccl_comm_destroy(ncclComm_t comm)
{
    const ncclResult_t inj = counted("ncclCommDestroy", sim::FN_RELEASE);
    Books &b = B();
    CommRec *c = live_comm(comm, "ncclCommDestroy");
    if (!c) return ncclInvalidArgument;
    // (an injected failure is reported and the registration goes all the same: comm.cpp cannot call again, it has deleted its handle)
    for (auto &kv : b.wait)
        for (std::deque<Pending> *q : {&kv.second.first, &kv.second.second})
            for (auto it = q->begin(); it != q->end();) it = it->comm == c ? q->erase(it) : it + 1;
    b.comms.erase(c);
    delete c;
    return inj;
}

ncclResult_t fake_rccl_group_start(void)
{
    if (ncclResult_t e = counted("ncclGroupStart", sim::FN_OTHER)) return e;
    ++B().depth;
    return ncclSuccess;
}

ncclResult_t fake_rccl_group_end(void)
{
    const ncclResult_t inj = counted("ncclGroupEnd", sim::FN_OTHER);
    Books &b = B();
    if (b.depth == 0) { sim::violation(sim::V_CHECK, "ncclGroupEnd without an ncclGroupStart"); return ncclInvalidUsage; }
    if (--b.depth) return inj;
    if (inj || b.group_failed) {  // closed, and nothing of it starts
        b.group.clear();
        b.group_failed = false;
        return inj ? inj : ncclInternalError;
    }
    submit();
    return ncclSuccess;
}

ncclResult_t fake_rccl_send(const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    return operation("ncclSend", true, buf, count, type, peer, comm, stream);
}
ncclResult_t fake_rccl_recv(void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    return operation("ncclRecv", false, buf, count, type, peer, comm, stream);
}

const char *fake_rccl_error_string(ncclResult_t e)
{
    ++g_calls;
    switch (e) {
        case ncclSuccess: return "no error";
        case ncclUnhandledCudaError: return "unhandled cuda error (simulated)";
        case ncclSystemError: return "unhandled system error (simulated)";
        case ncclInternalError: return "internal error (simulated)";
        case ncclInvalidArgument: return "invalid argument (simulated)";
        case ncclInvalidUsage: return "invalid usage (simulated)";
        default: return "unknown result code (simulated)";
    }
}

}  // extern "C"
#endif
