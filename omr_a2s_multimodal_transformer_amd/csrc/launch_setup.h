// One-time launch set-up of a kernel instantiation (host side), shared by every launcher of the library.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>

constexpr int OMR_NUM_CU = 256;   // compute units of an MI355X: the unit of every persistent grid

// Opt `kern` in to `shm` bytes of dynamic LDS (when `opt_in`) and, with block > 0, look up how many `block`-thread workgroups
// of it a CU holds (`fallback_occ` when the query fails).  Both are done once per `once`, a function-local static of the
// calling instantiation whose only transition is 0 -> value: racing first calls compute the same value (one process drives
// one GPU).  Returns that value (>= 1; 1 without a block size), or 0 when the opt-in was refused.
inline int omr_launch_setup(std::atomic<int>& once, const void* kern, size_t shm, bool opt_in, int block = 0, int fallback_occ = 1) {
    int v = once.load(std::memory_order_acquire);
    if (v) return v;
    if (opt_in && hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess) return 0;
    v = 1;
    if (block > 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kern, block, shm) != hipSuccess || v < 1)) v = fallback_occ;
    once.store(v, std::memory_order_release);
    return v;
}
