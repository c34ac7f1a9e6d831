// xsd_mem.hip -- xsd::dev_alloc / xsd::dev_free (xsd_mem.h): the only hipMalloc and the only hipFree of the library, each beside its
// ledger entry (xsd_ledger.h).  Host code only, no kernel lives here.
#include <hip/hip_runtime.h>

#include "xsd_ledger.h"
#include "xsd_mem.h"

namespace xsd {

static Ledger& ledger()
{
    static Ledger* l = new Ledger();      // never destroyed: handles may be freed from static destructors of the host program
    return *l;
}

hipError_t dev_alloc(void** p, size_t bytes)
{
    *p = nullptr;
    if (!ledger().admit()) return hipErrorOutOfMemory;
    const hipError_t err = hipMalloc(p, bytes);
    if (err != hipSuccess) { *p = nullptr; return err; }
    ledger().add(*p, bytes);
    return hipSuccess;
}

hipError_t dev_free(void* p)
{
    if (!p) return hipSuccess;
    ledger().remove(p);       // a pointer the ledger does not know is counted (foreign_frees) and still handed to the runtime
    return hipFree(p);
}

void mem_stats(int64_t out[6])
{
    const LedgerStats s = ledger().stats();
    out[0] = s.live_blocks; out[1] = s.live_bytes; out[2] = s.allocs; out[3] = s.frees; out[4] = s.foreign_frees; out[5] = s.refused;
}

int64_t mem_refuse(int64_t nth) { return ledger().refuse_nth(nth); }

} // namespace xsd
