// Host thread pool shared by the pipeline workers (host_pool.h).  A worker's host phases (hits from chains, DP-window planning,
// CIGAR stitching, MAPQ/text) are short bursts between GPU waits; with a private share of the cores a worker would crawl
// through its burst while the threads of the workers that wait on the GPU sleep.  Every burst is a job in one queue and
// every idle pool thread helps the oldest open job; the posting thread works on its own job too, so a job always
// advances.  fn(i, slot): slot < max_par identifies the helping thread (per-thread accumulators of the caller).
#include "host_pool.h"

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>

namespace mpn {

bool g_cpu_on = false;
std::atomic<long long> g_cpu_ns[32];

void CpuSect::lap(int k) {
    if (!on) return;
    timespec b;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &b);
    g_cpu_ns[16 + k] += (b.tv_sec - t.tv_sec) * 1000000000LL + (b.tv_nsec - t.tv_nsec);
    t = b;
}

namespace {
class HostPool {
    struct Job {
        const std::function<void(int, int)> *fn;
        int n, max_par, tag = 0, chunk = 1;   // items are handed out `chunk` at a time: one atomic per item is a hot cache line
        std::atomic<int> next{0};
        int slots = 1, active = 0;  // guarded by mu (slot 0 is the posting thread)
    };
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<Job *> jobs;
    std::vector<std::thread> threads;
    bool stop = false;

    static void drain(Job &j, int slot) {
        for (;;) {
            const int i0 = j.next.fetch_add(j.chunk);
            if (i0 >= j.n) break;
            const int i1 = std::min(j.n, i0 + j.chunk);
            for (int i = i0; i < i1; ++i) (*j.fn)(i, slot);
        }
    }
    static void run(Job &j, int slot) {
        if (!g_cpu_on) { drain(j, slot); return; }
        timespec a, b;
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &a);
        drain(j, slot);
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &b);
        g_cpu_ns[j.tag & 31] += (b.tv_sec - a.tv_sec) * 1000000000LL + (b.tv_nsec - a.tv_nsec);
    }
    Job *pick(int *slot) {  // mu held
        for (Job *j : jobs)
            if (j->slots < j->max_par && j->next.load(std::memory_order_relaxed) < j->n) { *slot = j->slots++; ++j->active; return j; }
        return nullptr;
    }
    void worker() {
        pthread_setname_np(pthread_self(), "mpn-pool");
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            int slot = 0;
            Job *j = nullptr;
            cv_work.wait(lk, [&]() { return stop || (j = pick(&slot)) != nullptr; });
            if (stop) return;
            lk.unlock();
            run(*j, slot);
            lk.lock();
            if (--j->active == 0) cv_done.notify_all();
        }
    }

public:
    void ensure(int n_threads) {
        std::lock_guard<std::mutex> g(mu);
        while ((int)threads.size() < n_threads - 1) threads.emplace_back([this]() { worker(); });
    }
    // grain: items that are worth one helping thread.  The bursts of a sub-batch are a few thousand light items: waking all
    // pool threads for each of them (a futex round trip and a fight for the queue lock per thread and burst) cost more CPU
    // than the items themselves.
    void parallel_for(int n, int max_par, const std::function<void(int, int)> &fn, int tag = 0, int grain = 512) {
        max_par = std::min(max_par, 1 + n / std::max(1, grain));
        if (max_par <= 1 || n < 2) { for (int i = 0; i < n; ++i) fn(i, 0); return; }
        Job j;
        j.fn = &fn; j.n = n; j.max_par = max_par; j.tag = tag;
        j.chunk = std::max(1, std::min(32, n / (max_par * 8)));
        { std::lock_guard<std::mutex> g(mu); jobs.push_back(&j); }
        for (int k = 1; k < max_par; ++k) cv_work.notify_one();
        run(j, 0);
        std::unique_lock<std::mutex> lk(mu);
        for (auto it = jobs.begin(); it != jobs.end(); ++it) if (*it == &j) { jobs.erase(it); break; }
        cv_done.wait(lk, [&]() { return j.active == 0; });
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv_work.notify_all();
        for (auto &t : threads) t.join();
    }
};
HostPool g_pool;
}  // namespace

void pool_ensure(int n_threads) { g_pool.ensure(n_threads); }

void parallel_for(int n, int n_threads, const std::function<void(int, int)> &fn, int tag, int grain) { g_pool.parallel_for(n, n_threads, fn, tag, grain); }

void parallel_chunks(int64_t n, int n_threads, const std::function<void(int64_t, int64_t, int)> &fn, int tag) {
    if (n_threads <= 1 || n < 8192) { fn(0, n, 0); return; }
    g_pool.parallel_for(n_threads, n_threads, [&](int t, int) { fn(n * t / n_threads, n * (t + 1) / n_threads, t); }, tag, 1);
}

int default_host_threads(const mpn_map_opt *opt) {
    if (const char *e = getenv("MPN_HOST_THREADS")) return std::max(1, atoi(e));
    if (opt->host_threads > 0) return opt->host_threads;
    static const int detected = []() {
        long long cores = std::max(1, (int)std::thread::hardware_concurrency());
        long long quota = -1, period = 100000;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[64] = {0};
            if (fscanf(f, "%63s %lld", q, &period) >= 1 && strcmp(q, "max") != 0) quota = atoll(q);
            fclose(f);
        } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
            if (fscanf(g, "%lld", &quota) != 1) quota = -1;
            fclose(g);
            if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(h, "%lld", &period) != 1) period = 100000; fclose(h); }
        }
        if (quota > 0 && period > 0) cores = std::min(cores, std::max(1LL, (quota + period - 1) / period));
        // one process per GPU: the ranks of a node share its cores (bench.py / the launcher export the rank count)
        int ranks = 1;
        if (const char *e = getenv("MPN_RANKS_ON_NODE")) ranks = std::max(1, atoi(e));
        else if (const char *e2 = getenv("LOCAL_WORLD_SIZE")) ranks = std::max(1, atoi(e2));
        // twice this rank's share of the cores, at most 32: the pool's threads mostly serve short bursts between GPU waits, and a
        // burst waiting for a free pool thread costs more than the quota's throttling (measured on a 16-CPU quota, one rank:
        // 16 threads 84.7, 24: 86.4, 32: 88.2, 48: 84.1 Gbp/min); never fewer than 4 (a rank's host phases need ~4 cores)
        const int n = (int)std::max(4LL, std::min(32LL, 2 * cores / ranks));
        return n;
    }();
    return detected;
}

}  // namespace mpn
