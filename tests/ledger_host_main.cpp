// Stand-alone program over csrc/xsd_ledger.h (tests/test_mem_ledger_host.py builds and runs it; no HIP, no device): prints one
// "name value" line per check and exits 0 only when every check holds.
#include <cstdio>
#include <thread>
#include <vector>

#include "xsd_ledger.h"

static int failures = 0;
#define CHECK(cond) do { const bool ok_ = (cond); std::printf("%s %s\n", ok_ ? "ok  " : "FAIL", #cond); if (!ok_) ++failures; } while (0)

static bool same(const xsd::LedgerStats& s, int64_t blocks, int64_t bytes, int64_t allocs, int64_t frees, int64_t foreign, int64_t refused)
{
    return s.live_blocks == blocks && s.live_bytes == bytes && s.allocs == allocs && s.frees == frees && s.foreign_frees == foreign && s.refused == refused;
}

int main()
{
    char mem[8];
    {   // add / remove, a foreign free, a second free of the same pointer, the null free
        xsd::Ledger l;
        CHECK(same(l.stats(), 0, 0, 0, 0, 0, 0));
        CHECK(l.admit());
        l.add(mem + 0, 100);
        CHECK(l.admit());
        l.add(mem + 1, 28);
        CHECK(same(l.stats(), 2, 128, 2, 0, 0, 0));
        CHECK(l.remove(mem + 0));
        CHECK(same(l.stats(), 1, 28, 2, 1, 0, 0));
        CHECK(!l.remove(mem + 0));                         // already taken back: foreign now
        CHECK(!l.remove(mem + 5));                         // never handed out
        CHECK(same(l.stats(), 1, 28, 2, 1, 2, 0));
        CHECK(l.remove(nullptr));                          // a no-op and not foreign
        CHECK(same(l.stats(), 1, 28, 2, 1, 2, 0));
        CHECK(l.remove(mem + 1));
        CHECK(same(l.stats(), 0, 0, 2, 2, 2, 0));
        l.add(mem + 2, 0);                                 // a zero-byte block is a block
        CHECK(same(l.stats(), 1, 0, 3, 2, 2, 0));
        CHECK(l.remove(mem + 2));
    }
    {   // refuse-at-nth fires exactly once; the return value counts the attempts since the previous arming
        xsd::Ledger l;
        CHECK(l.refuse_nth(3) == 0);
        CHECK(l.admit());
        CHECK(l.admit());
        CHECK(!l.admit());
        CHECK(l.stats().refused == 1);
        for (int i = 0; i < 10; ++i) CHECK(l.admit());     // spent: never again
        CHECK(l.stats().refused == 1);
        CHECK(l.refuse_nth(1) == 13);                      // 3 + 10 attempts, the refused one among them
        CHECK(!l.admit());
        CHECK(l.admit());
        CHECK(l.stats().refused == 2);
        CHECK(l.refuse_nth(2) == 2);
        CHECK(l.admit());
        CHECK(l.refuse_nth(0) == 1);                       // a disarm: the armed second attempt passes
        CHECK(l.admit());
        CHECK(l.admit());
        CHECK(l.stats().refused == 2);
        CHECK(l.refuse_nth(-5) == 2);                      // a negative count disarms too
        CHECK(l.admit());
        CHECK(l.stats().allocs == 0 && l.stats().live_blocks == 0);      // admit alone hands nothing out
    }
    {   // two threads allocating and freeing concurrently: exact final counters
        xsd::Ledger l;
        constexpr int N = 20000, KEEP = 7;
        static char arena[2][N];
        auto work = [&](int t) {
            for (int i = 0; i < N; ++i) {
                if (!l.admit()) continue;
                l.add(&arena[t][i], (size_t)(i % 13 + 1));
                if (i % KEEP) l.remove(&arena[t][i]);
                l.remove(nullptr);
            }
        };
        std::thread a(work, 0), b(work, 1);
        a.join();
        b.join();
        int64_t kept = 0, kept_bytes = 0;
        for (int i = 0; i < N; ++i)
            if (i % KEEP == 0) { ++kept; kept_bytes += i % 13 + 1; }
        CHECK(same(l.stats(), 2 * kept, 2 * kept_bytes, 2 * N, 2 * (N - kept), 0, 0));
        CHECK(l.refuse_nth(0) == 2 * N);
        for (int t = 0; t < 2; ++t)
            for (int i = 0; i < N; i += KEEP) l.remove(&arena[t][i]);
        CHECK(same(l.stats(), 0, 0, 2 * N, 2 * N, 0, 0));
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "PASSED", failures);
    return failures ? 1 : 0;
}
