// The owners of the library's GPU resources (host side only): device buffers, pinned host buffers, events and streams.
//
// Each is move-only and hands its resource back in its destructor, so a handle (bdx_ctx, bdx_bamdec, bdx_dist) or a one-shot entry point
// frees what it holds by going out of scope, on every path.  NO object of these types may have static or thread storage duration: its
// destructor would run after the HIP runtime has shut down, which is a crash at process exit.  They live in handles and on the stack.
#pragma once
#include <hip/hip_runtime.h>

#include <sys/mman.h>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace bdx {

// BDX_ALLOC_TRACE=1: every allocation of these buffers with its size and duration, and every free with its size, on stderr
inline bool alloc_trace() { static const bool on = getenv("BDX_ALLOC_TRACE") != nullptr; return on; }

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t b) {
        if (b <= bytes) return hipSuccess;
        const auto t0 = std::chrono::steady_clock::now();
        const bool had = p != nullptr;
        release();   // (waits for the device to go idle: steady-state code must not get here; under the trace the interval timed here takes in the free line's fprintf)
        size_t want = b + b / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (alloc_trace()) fprintf(stderr, "[bdx alloc] device %12zu B %8.1f us%s\n", want, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), had ? " (regrown: hipFree first)" : "");
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            if (alloc_trace()) fprintf(stderr, "[bdx free] device %12zu B\n", bytes);
        }
        p = nullptr; bytes = 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // A large buffer is anonymous memory on transparent huge pages, registered with the runtime (hipHostRegister): 0.02 s per 0.5 GB
    // against hipHostMalloc's 0.09-0.11 -- pinning is paid per page -- and a quarter less to hand back when the process ends
    // (tools/pin_probe.hip, profiles/r05_pin_probe.txt); the device sees it at the same address.  Small buffers -- the words the host
    // polls, the records kernels and host exchange mid-run -- stay with hipHostMalloc (fine-grained by default).  bdx_set_process_option("pin_malloc", 1): all of them.
    void* map_base = nullptr;
    size_t map_len = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept { take(o); }
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) { release(); take(o); }
        return *this;
    }
    ~PinBuf() { release(); }
    static std::atomic<bool>& registered_switch() { static std::atomic<bool> on{true}; return on; }   // bdx_set_process_option("pin_malloc", 1) turns it off
    static bool use_registered() { return registered_switch().load(std::memory_order_relaxed); }
    hipError_t ensure(size_t b) {
        if (b <= bytes) return hipSuccess;
        const bool had = p != nullptr;
        release();
        size_t want = b + b / 8 + 256;
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e = hipErrorOutOfMemory;
        constexpr size_t kHuge = (size_t)2 << 20;
        if (want >= 2 * kHuge && use_registered()) {
            const size_t len = (want + kHuge - 1) & ~(kHuge - 1);
            void* base = mmap(nullptr, len + kHuge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (base != MAP_FAILED) {
                void* al = (void*)(((uintptr_t)base + kHuge - 1) & ~(uintptr_t)(kHuge - 1));
                (void)madvise(al, len, MADV_HUGEPAGE);
                for (size_t o = 0; o < len; o += 4096) ((volatile char*)al)[o] = 0;   // (faulted in before it is pinned: one fault per huge page)
                void* dev = nullptr;
                if (hipHostRegister(al, len, hipHostRegisterMapped) == hipSuccess && hipHostGetDevicePointer(&dev, al, 0) == hipSuccess && dev == al) {
                    p = al; map_base = base; map_len = len + kHuge; want = len; e = hipSuccess;
                } else {
                    (void)hipHostUnregister(al);
                    (void)hipGetLastError();
                    munmap(base, len + kHuge);
                }
            }
        }
        if (e != hipSuccess) {
            e = hipHostMalloc(&p, want, hipHostMallocDefault);
            // (small buffers hold the words the host polls and the counters kernels report: a block the allocator hands out again may still
            // hold another context's ready word -- the same sequence number -- and a poll would return before the kernel has run)
            if (e == hipSuccess && want <= ((size_t)1 << 20)) memset(p, 0, want);
        }
        if (alloc_trace()) fprintf(stderr, "[bdx alloc] pinned %12zu B %8.1f us%s%s\n", want, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), map_base ? " (registered huge pages)" : "", had ? " (regrown: freed first)" : "");
        if (e == hipSuccess) bytes = want; else p = nullptr;
        return e;
    }
    void release() {
        if (p && map_base) { (void)hipHostUnregister(p); munmap(map_base, map_len); }
        else if (p) (void)hipHostFree(p);
        if (p && alloc_trace()) fprintf(stderr, "[bdx free] pinned %12zu B\n", bytes);
        p = nullptr; bytes = 0; map_base = nullptr; map_len = 0;
    }
    template <class T> T* as() const { return (T*)p; }

private:
    void take(PinBuf& o) {
        p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0);
        map_base = std::exchange(o.map_base, nullptr); map_len = std::exchange(o.map_len, 0);
    }
};

// A HIP event.  Converts to the raw handle, so it goes wherever a hipEvent_t goes.  create() without an argument is hipEventCreate
// (which is hipEventCreateWithFlags(hipEventDefault)): an event that can be timed; a stream has no such default, its flags are always given.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { reset(); e = std::exchange(o.e, nullptr); }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&e, flags); }
    void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

// A HIP stream: one of its own (create) or one that belongs to somebody else (borrow), which the destructor leaves alone.
struct Stream {
    hipStream_t s = nullptr;
    bool owned = false;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)), owned(std::exchange(o.owned, false)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) { reset(); s = std::exchange(o.s, nullptr); owned = std::exchange(o.owned, false); }
        return *this;
    }
    ~Stream() { reset(); }
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        owned = e == hipSuccess;
        return e;
    }
    void borrow(hipStream_t other) { reset(); s = other; }
    void reset() { if (s && owned) (void)hipStreamDestroy(s); s = nullptr; owned = false; }
    operator hipStream_t() const { return s; }
};

}  // namespace bdx
