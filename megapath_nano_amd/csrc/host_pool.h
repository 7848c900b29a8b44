// Host thread pool shared by the pipeline workers, and the thread-CPU accounting of its parallel regions (MPN_DEBUG_CPU).
// Host only: no HIP include.
#pragma once
#include "../../include/mpn_map.h"

#include <atomic>
#include <functional>
#include <stdint.h>
#include <time.h>

namespace mpn {

extern bool g_cpu_on;                      // MPN_DEBUG_CPU=1: thread CPU time of every parallel region, by tag
extern std::atomic<long long> g_cpu_ns[32];

// MPN_DEBUG_CPU: thread CPU time of the sections of a host phase (g_cpu_ns[16 + k])
struct CpuSect {
    timespec t;
    bool on;
    explicit CpuSect(bool o) : on(o) { if (on) clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t); }
    void lap(int k);
};

// Threads of the host pool: what the caller asks for, else the cores this process may actually use -- the container's CPU
// quota (cgroup v2 cpu.max / v1 cfs quota) counts, not just the visible cores: with 256 visible cores and a quota of 16
// a pool sized by the visible cores is throttled -- capped at 32.
int default_host_threads(const mpn_map_opt *opt);
// the pool has at least n_threads - 1 threads from here on (the posting thread is the n-th)
void pool_ensure(int n_threads);
// fn(i, slot) for every i < n on up to n_threads threads; slot < n_threads identifies the helping thread (per-thread accumulators
// of the caller).  grain: items that are worth one helping thread; tag: the g_cpu_ns slot the region is charged to.
void parallel_for(int n, int n_threads, const std::function<void(int, int)> &fn, int tag = 0, int grain = 512);
// fn(lo, hi, t): chunk t of n_threads equal ranges of [0, n); the chunk index is what the callers use for their per-thread accumulators
void parallel_chunks(int64_t n, int n_threads, const std::function<void(int64_t, int64_t, int)> &fn, int tag = 0);

}  // namespace mpn
