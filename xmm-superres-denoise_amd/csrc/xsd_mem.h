// xsd_mem.h -- the library's one way to device memory: every translation unit allocates with xsd::dev_alloc and frees with
// xsd::dev_free, so that what the library holds is on one account (xsd_ledger.h; read through xsd_test_mem_stats of include/xsd.h).
// No hipMalloc / hipFree call stands anywhere else under csrc/ (tests/test_mem_one_copy.py).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace xsd {
// hipMalloc through the ledger.  On failure *p is null.  When the refusal armed by xsd_test_mem_refuse fires, answers
// hipErrorOutOfMemory without calling the runtime (nothing to clear with hipGetLastError).  Defined in xsd_mem.hip; hidden.
__attribute__((visibility("hidden"))) hipError_t dev_alloc(void** p, size_t bytes);
template <class T> inline hipError_t dev_alloc(T** p, size_t bytes) { return dev_alloc(reinterpret_cast<void**>(p), bytes); }
// hipFree through the ledger; nullptr is a no-op, as for hipFree.
__attribute__((visibility("hidden"))) hipError_t dev_free(void* p);
// the test entries' access to the account (xsd_test_entries.hip)
__attribute__((visibility("hidden"))) void mem_stats(int64_t out[6]);      // live_blocks, live_bytes, allocs, frees, foreign_frees, refused
__attribute__((visibility("hidden"))) int64_t mem_refuse(int64_t nth);
}
