// lbm_mem.h -- the one place that allocates and frees device and pinned host memory. Host only.
// A MemPool remembers every block it hands out and frees what is left when it dies: a handle, the background writers and the
// communicator each have one for what lives as long as they do; a function that needs scratch for one call has a local one,
// so that no early return leaks. One hipMalloc / hipHostMalloc per request: no arena, nothing cached.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <atomic>
#include <vector>

class MemPool {   // not copyable; not thread-safe: one owner thread at a time
 public:
  MemPool() = default;
  MemPool(const MemPool&) = delete;
  MemPool& operator=(const MemPool&) = delete;
  ~MemPool() { release_all(); }

  // A request of 0 bytes becomes 16. On failure *p stays null and nothing is remembered.
  hipError_t dev(void** p, size_t bytes) { return take(p, bytes, false); }
  hipError_t pinned(void** p, size_t bytes) { return take(p, bytes, true); }   // hipHostMallocDefault
  template <class T> hipError_t dev(T** p, size_t count) { return take((void**)p, sizeof(T) * count, false); }
  template <class T> hipError_t pinned(T** p, size_t count) { return take((void**)p, sizeof(T) * count, true); }

  // A device block that is kept from call to call and only grows: nothing happens while *p holds `want` elements; otherwise the
  // old block goes and one of exactly `want` elements comes (on failure *p is null and *cap 0). The caller chooses `want`.
  template <class T> hipError_t grow(T** p, long* cap, long want) {
    if (*p && *cap >= want) return hipSuccess;
    release(*p);
    *p = nullptr; *cap = 0;
    const hipError_t e = dev(p, (size_t)want);
    if (e == hipSuccess) *cap = want;
    return e;
  }

  // frees and forgets ONE block; null (and a pointer the pool does not know) is a no-op
  void release(const volatile void* p) {
    for (size_t k = blocks_.size(); p && k-- > 0;)
      if (blocks_[k].p == p) {
        drop(blocks_[k]);
        blocks_.erase(blocks_.begin() + (long)k);
        return;
      }
  }
  // frees what is left, newest first
  void release_all() {
    for (; !blocks_.empty(); blocks_.pop_back()) drop(blocks_.back());
  }

  // process-wide: blocks handed out and not yet freed, and their requested bytes (after the 0 -> 16 rule)
  static std::atomic<long>& live_blocks() { static std::atomic<long> v{0}; return v; }
  static std::atomic<long>& live_bytes() { static std::atomic<long> v{0}; return v; }

 private:
  struct Block { void* p; size_t bytes; bool pinned; };
  std::vector<Block> blocks_;

  hipError_t take(void** p, size_t bytes, bool pinned) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    blocks_.reserve(blocks_.size() + 1);   // (a host bad_alloc comes before the block exists, not after)
    void* q = nullptr;
    const hipError_t e = pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();   // (the caller has the error: a hipGetLastError() behind a later launch must not find it again)
      return e;
    }
    blocks_.push_back(Block{q, bytes, pinned});
    live_blocks() += 1;
    live_bytes() += (long)bytes;
    *p = q;
    return hipSuccess;
  }
  static void drop(const Block& b) {
    if (b.pinned) (void)hipHostFree(b.p); else (void)hipFree(b.p);
    live_blocks() -= 1;
    live_bytes() -= (long)b.bytes;
  }
};
