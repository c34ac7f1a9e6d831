// xsd_ledger.h -- the account of what the library holds on the device: every allocation xsd::dev_alloc hands out and every pointer
// xsd::dev_free takes back (xsd_mem.h) passes through one Ledger.  Plain C++17, no HIP: the unit test compiles it with g++ alone.
//
// The ledger only counts.  It never calls the runtime and never refuses a free; the one decision it makes is the armed refusal
// (refuse_nth): the n-th admit() from the arming answers false, once, and the caller fails as for a device that is out of memory.
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <unordered_map>

namespace xsd {

struct LedgerStats {
    int64_t live_blocks = 0;       // allocations handed out and not yet freed
    int64_t live_bytes = 0;        // their sizes as asked for
    int64_t allocs = 0;            // add() calls since the library was loaded
    int64_t frees = 0;             // remove() calls that found their pointer
    int64_t foreign_frees = 0;     // remove() of a non-null pointer the ledger never handed out (or handed out and already took back)
    int64_t refused = 0;           // admit() calls answered false
};

class __attribute__((visibility("hidden"))) Ledger {
public:
    // Before an allocation: false = refuse it (the armed one), without touching the runtime.  Counts the attempt either way.
    bool admit()
    {
        std::lock_guard<std::mutex> g(mu_);
        ++since_arm_;
        if (arm_ > 0 && --arm_ == 0) { ++st_.refused; return false; }
        return true;
    }
    // After the runtime handed `p` out.
    void add(const void* p, size_t bytes)
    {
        std::lock_guard<std::mutex> g(mu_);
        ++st_.allocs;
        auto it = live_.find(p);
        if (it != live_.end()) { st_.live_bytes -= (int64_t)it->second; it->second = bytes; }      // (a runtime that hands out a live pointer twice: keep one entry)
        else { live_.emplace(p, bytes); ++st_.live_blocks; }
        st_.live_bytes += (int64_t)bytes;
    }
    // Before the runtime takes `p` back.  nullptr: nothing, as for free(); true = the pointer was the ledger's.
    bool remove(const void* p)
    {
        if (!p) return true;
        std::lock_guard<std::mutex> g(mu_);
        auto it = live_.find(p);
        if (it == live_.end()) { ++st_.foreign_frees; return false; }
        ++st_.frees; --st_.live_blocks; st_.live_bytes -= (int64_t)it->second;
        live_.erase(it);
        return true;
    }
    // nth >= 1: the nth admit() from now answers false, once; 0 disarms.  Returns the admit() calls since the previous refuse_nth.
    int64_t refuse_nth(int64_t nth)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t made = since_arm_;
        since_arm_ = 0;
        arm_ = nth > 0 ? nth : 0;
        return made;
    }
    LedgerStats stats() const
    {
        std::lock_guard<std::mutex> g(mu_);
        return st_;
    }

private:
    mutable std::mutex mu_;
    std::unordered_map<const void*, size_t> live_;
    LedgerStats st_;
    int64_t arm_ = 0, since_arm_ = 0;
};

} // namespace xsd
