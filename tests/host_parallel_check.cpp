// Stand-alone check of ds2i_amd/csrc/host_parallel.hpp (tests/test_host_parallel_cpu.py compiles and runs it; it also builds with
// -fsanitize=thread and with -fsanitize=address,undefined). One line per case on stdout, "FAIL ..." and exit status 1 if one does not hold.
#include <atomic>
#include <cstdio>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../ds2i_amd/csrc/host_parallel.hpp"

using ds2i_host::parallel_for;

namespace {
int failures = 0;
void expect(bool ok, const char* what, uint64_t n, unsigned threads, bool caller) {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s (n=%llu threads=%u caller_takes_part=%d)\n", what, (unsigned long long)n, threads, (int)caller);
}

// threads that ran fn and have ended since: a worker counts itself in when it first runs fn and out when the thread ends (the destructor
// of a thread_local runs before join() returns)
std::atomic<int> workers_started(0), workers_ended(0);
struct WorkerLife {
    WorkerLife() { ++workers_started; }
    ~WorkerLife() { ++workers_ended; }
};
void mark_worker(bool is_caller) {
    if (is_caller) return; // (the calling thread outlives the call)
    thread_local WorkerLife life;
    (void)life;
}

// every index once, worker numbers inside [0, threads), a worker's scratch slot is its own
void visits(uint64_t n, unsigned threads, bool caller) {
    std::vector<std::atomic<uint32_t>> seen(n);
    for (auto& s : seen) s = 0;
    std::vector<uint64_t> scratch(threads, 0); // plain words: a slot shared by two threads is a data race the thread sanitizer reports
    std::atomic<bool> bad_worker(false), wrong_thread(false);
    const std::thread::id me = std::this_thread::get_id();
    workers_started = workers_ended = 0;
    parallel_for(n, threads, [&](uint64_t i, unsigned w) {
        if (w >= threads) { bad_worker = true; return; }
        const bool is_caller = std::this_thread::get_id() == me;
        mark_worker(is_caller);
        if (is_caller != (caller && w == 0)) wrong_thread = true; // worker 0 is the caller iff it takes part; nobody else ever is
        ++seen[i];
        ++scratch[w];
    }, caller);
    bool once = true;
    for (auto& s : seen) once = once && s == 1;
    uint64_t total = 0;
    for (uint64_t c : scratch) total += c;
    expect(once, "every index exactly once", n, threads, caller);
    expect(total == n, "the workers' counts add up to n", n, threads, caller);
    expect(!bad_worker, "worker numbers inside [0, threads)", n, threads, caller);
    expect(!wrong_thread, "the caller is worker 0 iff it takes part", n, threads, caller);
    expect(workers_started == workers_ended, "every worker joined", n, threads, caller);
    std::printf("visits n=%llu threads=%u caller_takes_part=%d\n", (unsigned long long)n, threads, (int)caller);
}

// an exception at one index: the caller gets its message, after every worker has joined, and no index ran twice
template <class Throw>
void throws(uint64_t n, unsigned threads, bool caller, uint64_t at, Throw thrower, const std::string& message) {
    std::vector<std::atomic<uint32_t>> seen(n);
    for (auto& s : seen) s = 0;
    const std::thread::id me = std::this_thread::get_id();
    workers_started = workers_ended = 0;
    bool caught = false;
    try {
        parallel_for(n, threads, [&](uint64_t i, unsigned) {
            mark_worker(std::this_thread::get_id() == me);
            ++seen[i];
            if (i == at) thrower();
        }, caller);
    } catch (std::exception const& e) {
        caught = true;
        expect(workers_started == workers_ended, "every worker joined before the exception reached the caller", n, threads, caller);
        expect(message == e.what(), "the exception's message reaches the caller", n, threads, caller);
    }
    bool at_most_once = true;
    for (auto& s : seen) at_most_once = at_most_once && s <= 1;
    expect(caught, "the exception reaches the caller", n, threads, caller);
    expect(seen[at] == 1, "the throwing index ran", n, threads, caller);
    expect(at_most_once, "no index twice", n, threads, caller);
    std::printf("throws n=%llu threads=%u caller_takes_part=%d\n", (unsigned long long)n, threads, (int)caller);
}
} // namespace

int main() {
    for (unsigned threads : {1u, 3u, 16u})
        for (bool caller : {false, true}) {
            for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(threads - 1), uint64_t(threads + 1), uint64_t(1000)}) visits(n, threads, caller);
            throws(1000, threads, caller, 137, [] { throw std::runtime_error("boom at 137"); }, "boom at 137");
            throws(1000, threads, caller, 0, [] { throw std::bad_alloc(); }, std::bad_alloc().what());
            throws(threads + 1, threads, caller, threads, [] { throw 42; }, "unknown exception on a worker thread");
        }
    if (failures) return 1;
    std::printf("host_parallel: all checks passed\n");
    return 0;
}
