// handles.h -- which stream / buffer / event handles belong to which context: the only owner of that link, without HIP.
//
// A handle may be freed after its context, from any thread, also while another thread destroys that context
// (include/fft_wgpu_amd.h, "Lifetimes": finalizers of a garbage-collected host).  So the link lives inside the handle (an
// intrusive list: attaching allocates nothing and cannot throw) and ONE process-wide mutex guards every list: a mutex inside
// the context would die with it under the feet of a handle that is just being freed.  Only this header locks that mutex, and
// nothing here calls HIP; a functor given to for_each must not either.  tools/handle_stress.cpp races these operations under
// ThreadSanitizer and AddressSanitizer on a CPU (tests/test_handles.py).
#pragma once
#include <cstddef>
#include <mutex>

struct fwa_ctx;

namespace fwa_int {

enum HandleKind : int { H_STREAM = 0, H_BUF = 1, H_EVENT = 2, H_KINDS = 3 };

struct HandleList;

// Base of fwa_stream, fwa_buf and fwa_event.  `ctx` is what the rest of the library reads (nullptr: the context is gone);
// `list` is set only while the handle is attached -- a plan's own second buffer carries a `ctx` but is never attached.
struct Handle {
    fwa_ctx *ctx = nullptr;
    HandleList *list = nullptr;
    Handle *prev = nullptr, *next = nullptr;
    HandleKind kind = H_KINDS;
};

// The one member of fwa_ctx that knows its alive handles, in creation order.
struct HandleList {
    Handle *head = nullptr, *tail = nullptr;
    std::ptrdiff_t n[H_KINDS] = {0, 0, 0};
};

inline std::mutex &registry_mutex() noexcept
{
    static std::mutex m;  // outlives every context
    return m;
}

// h is complete and not yet visible to any other thread
inline void attach(fwa_ctx *ctx, HandleList &list, Handle *h, HandleKind kind) noexcept
{
    std::lock_guard<std::mutex> lk(registry_mutex());
    h->ctx = ctx; h->list = &list; h->kind = kind;
    h->prev = list.tail; h->next = nullptr;
    (list.tail ? list.tail->next : list.head) = h;
    list.tail = h;
    ++list.n[kind];
}

// Before a handle is deleted.  Does nothing once the context has detached it (or if it never was attached).
inline void detach(Handle *h) noexcept
{
    std::lock_guard<std::mutex> lk(registry_mutex());
    HandleList *list = h->list;
    if (!h->ctx || !list) return;
    (h->prev ? h->prev->next : list->head) = h->next;
    (h->next ? h->next->prev : list->tail) = h->prev;
    --list->n[h->kind];
    h->ctx = nullptr; h->list = nullptr; h->prev = h->next = nullptr;
}

// Before a context is deleted: every handle of it answers "my context is gone" from here on.
inline void detach_all(HandleList &list) noexcept
{
    std::lock_guard<std::mutex> lk(registry_mutex());
    for (Handle *h = list.head, *nx; h; h = nx) {
        nx = h->next;
        h->ctx = nullptr; h->list = nullptr; h->prev = h->next = nullptr;
    }
    list = HandleList{};
}

inline std::ptrdiff_t count(const HandleList &list, HandleKind kind) noexcept
{
    std::lock_guard<std::mutex> lk(registry_mutex());
    return list.n[kind];
}

// f(const Handle *) on every attached handle of one kind, oldest first, under the lock: f copies out what it needs and
// returns -- no HIP call, no allocation, nothing that throws.
template <class F>
inline void for_each(const HandleList &list, HandleKind kind, F &&f) noexcept
{
    std::lock_guard<std::mutex> lk(registry_mutex());
    for (const Handle *h = list.head; h; h = h->next)
        if (h->kind == kind) f(h);
}

}  // namespace fwa_int
