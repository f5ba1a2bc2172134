// host_parallel.hpp -- the one host thread pool of the build side (no HIP): the index builders, the optimiser, the chunk directory of an
// upload and the planner of the Elias-Fano encoder all run "fn for every list, lists drawn off a counter". (The query path's plan pool,
// batch_plan.cpp, is a different kind -- persistent threads fed batch after batch -- and does not come through here.)
#pragma once
#include <atomic>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace ds2i_host {

// fn(i, worker) for every i in [0, n), each exactly once: `threads` workers, numbered 0 .. threads - 1, draw the indices off one atomic
// counter (so `fn` may keep per-worker scratch in `threads` slots allocated beside the call). caller_takes_part: the calling thread is
// worker 0 and threads - 1 are started; otherwise all `threads` are started and the caller waits.
// Every worker is joined before this returns or throws. A worker whose fn throws stops drawing, and the indices nobody has drawn yet are
// dropped; the first exception is then rethrown in the caller as a std::runtime_error with its what() -- whatever its type was, so the
// code an entry point returns for a failed worker does not depend on which thread the failure happened on.
template <class Fn>
void parallel_for(uint64_t n, unsigned threads, Fn&& fn, bool caller_takes_part = false) {
    if (!threads) threads = 1;
    std::atomic<uint64_t> next(0);
    std::mutex err_mu;
    std::string err;
    bool failed = false;
    auto worker = [&](unsigned w) {
        try {
            for (;;) {
                const uint64_t i = next.fetch_add(1);
                if (i >= n) break;
                fn(i, w);
            }
        } catch (...) {
            next.store(n); // nobody draws another index (the counter only grows from here: no index is handed out twice)
            std::string what = "unknown exception on a worker thread";
            try {
                throw;
            } catch (std::exception const& e) {
                what = e.what();
            } catch (...) {
            }
            std::lock_guard<std::mutex> g(err_mu);
            if (!failed) err = std::move(what);
            failed = true;
        }
    };
    std::vector<std::thread> pool;
    pool.reserve(threads);
    try {
        for (unsigned w = caller_takes_part ? 1 : 0; w < threads; ++w) pool.emplace_back(worker, w);
    } catch (...) { // a thread could not be started: the ones that were finish the work, unless none was and the caller does not work
        if (pool.empty() && !caller_takes_part) throw;
    }
    if (caller_takes_part) worker(0);
    for (auto& th : pool) th.join();
    if (failed) throw std::runtime_error(err);
}

} // namespace ds2i_host
