// Part of jjs_gpu.hip (included inside its anonymous namespace, ahead of engine_state.h): the move-only owners of what the
// engine allocates on a device -- device and pinned host memory, grow-only buffers over either, streams, events.  A member of
// one of these types needs no line in the tear-down; a local one needs no unwinding.
//
// WHEN AN OWNER MAY FREE.  No call path frees memory: hipFree / hipHostFree wait for every stream of the device, and launches in
// flight may still read a buffer that has been replaced.  A replaced or destroyed buffer is RETIRED (release(), replace():
// retire() in engine_state.h files it under the device `g`) and freed by jjs_trim / jjs_shutdown.  An owner's destructor, and
// free(), really free, so they may run only
//   - when the device has been drained: tear-down (free_device), jjs_trim; or
//   - when nothing was ever queued against the allocation, or what was has ended: a replacement that was never installed, the
//     build area and the unpublished copies of a registered object (their build stream is drained first).
#pragma once

int fail(int code, const char* fmt, ...);
void retire(void* p, bool host, size_t bytes);

// One allocation of device memory (hipMalloc) or pinned host memory (hipHostMalloc) and the bytes it was allocated with.
template <class T, bool Pinned>
class owned_mem {
    T* p_ = nullptr;
    size_t bytes_ = 0;
public:
    owned_mem() = default;
    owned_mem(const owned_mem&) = delete;
    owned_mem& operator=(const owned_mem&) = delete;
    owned_mem(owned_mem&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    owned_mem& operator=(owned_mem&& o) noexcept {
        if (this != &o) { (void)free(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~owned_mem() { (void)free(); }
    hipError_t alloc(size_t bytes) {       // of an empty owner; it stays empty when the allocation fails
        void* fresh = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&fresh, bytes, hipHostMallocDefault) : hipMalloc(&fresh, bytes);
        if (e == hipSuccess) { p_ = static_cast<T*>(fresh); bytes_ = bytes; }
        return e;
    }
    hipError_t free() {                    // see above for when; the owner keeps an allocation that could not be freed
        if (!p_) return hipSuccess;
        const hipError_t e = Pinned ? hipHostFree(p_) : hipFree(p_);
        if (e == hipSuccess) { p_ = nullptr; bytes_ = 0; }
        return e;
    }
    void release() {                       // launches in flight may still use it: retired, under the device `g`
        retire(p_, Pinned, bytes_);
        p_ = nullptr; bytes_ = 0;
    }
    void replace(owned_mem&& fresh) { release(); *this = std::move(fresh); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t bytes() const { return bytes_; }
};
template <class T> using device_mem = owned_mem<T, false>;
template <class T> using pinned_mem = owned_mem<T, true>;

// Grow-only buffers: the replacement is allocated first, the old buffer is retired with the bytes it had, then they swap.  No
// call waits for the device here.  The capacity a buffer takes: grown() of grown.h.
// What differs from buffer to buffer, declared with the member: the capacity is counted in units (items, or bytes), never less
// than min_units, and `cap` units are cap * unit_bytes + slack_bytes bytes.
struct growth_rule { size_t min_units = 0, unit_bytes = 1, slack_bytes = 0; };
template <class T, bool Pinned = false>
class grow_only {
    owned_mem<T, Pinned> mem_;
    size_t cap_ = 0;
    const growth_rule rule_;
    __attribute__((noinline)) int grow(size_t want) {                  // (rare: kept out of the callers)
        const size_t cap = grown(want < rule_.min_units ? rule_.min_units : want);
        owned_mem<T, Pinned> fresh;
        const hipError_t e = fresh.alloc(cap * rule_.unit_bytes + rule_.slack_bytes);
        if (e != hipSuccess)
            return fail(JJS_ERR_HIP, "%s: %s", Pinned ? "hipHostMalloc(reinterpret_cast<void**>(&fresh), cap, hipHostMallocDefault)"
                                                      : "hipMalloc(reinterpret_cast<void**>(&fresh), bytes)", hipGetErrorString(e));
        mem_.replace(std::move(fresh));
        cap_ = cap;
        return JJS_OK;
    }
public:
    explicit grow_only(growth_rule rule = {}) : rule_(rule) {}
    int ensure(size_t want) { return want <= cap_ ? JJS_OK : grow(want); }
    hipError_t free() {                                               // on a drained device only (see above): jjs_trim
        const hipError_t e = mem_.free();
        if (e == hipSuccess) cap_ = 0;
        return e;
    }
    size_t capacity() const { return cap_; }                          // in units
    size_t reported_bytes() const { return cap_ * rule_.unit_bytes; } // what jjs_memory_stats counts: the units, not the slack
    T* get() const { return mem_.get(); }
    operator T*() const { return mem_.get(); }
};

// A stream or an event.  They are created where the order of creation is decided (init_device); the destructor waits for the
// stream and destroys it.
class stream_owner {
    hipStream_t s_ = nullptr;
public:
    stream_owner() = default;
    stream_owner(const stream_owner&) = delete;
    stream_owner& operator=(const stream_owner&) = delete;
    ~stream_owner() {
        if (s_) { (void)hipStreamSynchronize(s_); (void)hipStreamDestroy(s_); }
    }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s_, flags); }
    hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(&s_, flags, priority); }
    operator hipStream_t() const { return s_; }
};
class event_owner {
    hipEvent_t e_ = nullptr;
public:
    event_owner() = default;
    event_owner(const event_owner&) = delete;
    event_owner& operator=(const event_owner&) = delete;
    ~event_owner() {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }
};
