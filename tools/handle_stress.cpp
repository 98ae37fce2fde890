// tools/handle_stress.cpp -- race the handle registry (fft_wgpu_amd/csrc/handles.h) on a CPU, no device and no HIP.
//
// Two kinds of round, `rounds` of each (argv[1], default 200), 4 worker threads with 64 handles each:
//   destroy  handles of all three kinds are attached to a fresh context; the workers detach and delete their share while one
//            more thread detaches them all and deletes the context -- finalizers of a garbage-collected host against
//            fwa_ctx_destroy.  A few handles survive the context and must have lost their link.
//   churn    the workers attach handles to one context and detach every other one again, while the main thread counts and
//            walks the list; nothing is destroyed until they are done.
// Counts per kind and list order (= creation order) are checked in between, an empty list and null links after every round.
// tests/test_handles.py builds this with -fsanitize=thread and with -fsanitize=address,undefined and wants both silent.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "handles.h"

using namespace fwa_int;

struct fwa_ctx { HandleList handles; };

struct Item : Handle {
    int owner = 0, seq = 0;  // creating thread, creation order within it
};

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "handle_stress.cpp:%d: %s failed\n", __LINE__, #cond); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

constexpr int THREADS = 4, PER_THREAD = 64, SURVIVORS = 6;

static HandleKind kind_of(int owner, int seq) { return (HandleKind)((owner + seq) % H_KINDS); }

// every kind: as many handles as expected, each linked to ctx, each owner's handles in the order it created them
static void check_list(const fwa_ctx *ctx, const std::ptrdiff_t want[H_KINDS])
{
    for (int k = 0; k < H_KINDS; ++k) {
        std::ptrdiff_t seen = 0;
        int last[THREADS + 1];
        bool ok = true;
        for (int &l : last) l = -1;
        for_each(ctx->handles, (HandleKind)k, [&](const Handle *h) {
            const Item *it = static_cast<const Item *>(h);
            ok = ok && it->ctx == ctx && it->kind == k && it->seq > last[it->owner];
            last[it->owner] = it->seq;
            ++seen;
        });
        CHECK(ok);
        CHECK(seen == want[k]);
        CHECK(count(ctx->handles, (HandleKind)k) == want[k]);
    }
}

static void check_empty(const HandleList &list)
{
    for (int k = 0; k < H_KINDS; ++k) CHECK(count(list, (HandleKind)k) == 0);
    CHECK(!list.head && !list.tail);  // nothing is attached any more: no other thread reaches the list
}

static void free_detached(Item *it)
{
    detach(it);
    CHECK(!it->ctx && !it->list && !it->prev && !it->next);
    delete it;
}

static void destroy_round()
{
    fwa_ctx *ctx = new fwa_ctx;
    std::vector<Item *> share[THREADS], survivors;
    std::ptrdiff_t want[H_KINDS] = {0, 0, 0};
    // one creator, so list order is `seq` order over all owners: owner THREADS are the survivors, spread through the list
    for (int i = 0, seq = 0; i < PER_THREAD; ++i)
        for (int t = 0; t <= THREADS; ++t) {
            if (t == THREADS && (i % 8 != 0 || (int)survivors.size() == SURVIVORS)) continue;
            Item *it = new Item;
            it->owner = t; it->seq = seq++;
            attach(ctx, ctx->handles, it, kind_of(t, i));
            ++want[kind_of(t, i)];
            (t == THREADS ? survivors : share[t]).push_back(it);
        }
    CHECK((int)survivors.size() == SURVIVORS);
    check_list(ctx, want);
    // a plan's own second buffer: it names its context but is never attached, detaching it changes nothing
    Item unattached;
    unattached.ctx = ctx;
    detach(&unattached);
    CHECK(unattached.ctx == ctx);
    check_list(ctx, want);

    std::atomic<bool> go{false};
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t)
        th.emplace_back([&, t] {
            while (!go.load()) std::this_thread::yield();
            for (Item *it : share[t]) free_detached(it);
        });
    th.emplace_back([&] {
        while (!go.load()) std::this_thread::yield();
        detach_all(ctx->handles);
        check_empty(ctx->handles);
        delete ctx;
    });
    go.store(true);
    for (auto &t : th) t.join();
    for (Item *it : survivors) {
        CHECK(!it->ctx && !it->list);
        free_detached(it);
    }
}

static void churn_round()
{
    fwa_ctx *ctx = new fwa_ctx;
    std::vector<Item *> kept[THREADS];
    std::atomic<bool> go{false};
    std::atomic<int> running{THREADS};
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t)
        th.emplace_back([&, t] {
            while (!go.load()) std::this_thread::yield();
            for (int i = 0; i < PER_THREAD; ++i) {
                Item *it = new Item;
                it->owner = t; it->seq = i;
                attach(ctx, ctx->handles, it, kind_of(t, i));
                if (i & 1) free_detached(it);
                else kept[t].push_back(it);
            }
            --running;
        });
    go.store(true);
    while (running.load()) {  // readers beside the writers: the counts stay within what can be attached
        std::ptrdiff_t seen = 0;
        for (int k = 0; k < H_KINDS; ++k) {
            for_each(ctx->handles, (HandleKind)k, [&](const Handle *) { ++seen; });
            CHECK(count(ctx->handles, (HandleKind)k) <= THREADS * PER_THREAD);
        }
        CHECK(seen <= THREADS * PER_THREAD);
    }
    for (auto &t : th) t.join();
    std::ptrdiff_t want[H_KINDS] = {0, 0, 0};
    for (int t = 0; t < THREADS; ++t)
        for (int i = 0; i < PER_THREAD; i += 2) ++want[kind_of(t, i)];
    check_list(ctx, want);
    for (int t = 0; t < THREADS; ++t)
        for (Item *it : kept[t]) {
            CHECK(it->ctx == ctx);
            free_detached(it);
        }
    check_empty(ctx->handles);
    delete ctx;
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    for (int r = 0; r < rounds; ++r) {
        destroy_round();
        churn_round();
    }
    std::printf("handle_stress: %d destroy rounds and %d churn rounds, %d threads x %d handles: ok\n", rounds, rounds, THREADS,
                PER_THREAD);
    return 0;
}
