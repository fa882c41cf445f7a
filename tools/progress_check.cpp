// progress_check.cpp -- the pipeline's Progress counter (csrc/zw_progress.h)
// on the CPU: ordering under contention and the "stopped" rules the lane
// scheduler relies on.  Prints "ok" and exits 0 when all hold.
//   g++ -O2 -std=c++17 -pthread -I image-webp_amd/csrc tools/progress_check.cpp
#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>
#include <vector>

#include "zw_progress.h"

static int fail(const char* what)
{
    printf("FAILED: %s\n", what);
    return 1;
}

int main()
{
    // U producers advance N times each, one consumer waits for 1..N on each in
    // turn (the lane thread and its uploaders): a wait never returns early
    {
        const int U = 3, N = 10000;
        std::vector<Progress> prog(U);
        std::vector<std::atomic<int>> done(U);
        for (auto& d : done) d = 0;
        std::vector<std::thread> th;
        for (int u = 0; u < U; u++)
            th.emplace_back([&, u] {
                for (int i = 0; i < N; i++) {
                    done[u].fetch_add(1, std::memory_order_release);
                    prog[u].advance();
                }
            });
        bool early = false, stopped = false;
        for (int k = 1; k <= N; k++)
            for (int u = 0; u < U; u++) {
                if (!prog[u].wait_for(k)) stopped = true;
                if (done[u].load(std::memory_order_acquire) < k) early = true;
            }
        for (auto& t : th) t.join();
        if (stopped) return fail("wait_for failed on a counter nobody stopped");
        if (early) return fail("wait_for returned before the value was reached");
    }
    // stop() from another thread releases a waiter blocked on a value never reached
    {
        Progress pr;
        pr.advance();
        std::atomic<int> res{-1};
        std::thread w([&] { res = pr.wait_for(5) ? 1 : 0; });
        std::this_thread::sleep_for(std::chrono::milliseconds(20));  // (let it block; either order must fail)
        if (res.load() != -1) return fail("wait_for(5) returned at value 1");
        pr.stop();
        w.join();
        if (res.load() != 0) return fail("a stopped wait_for returned true");
        pr.stop();  // idempotent
        if (pr.wait_for(1)) return fail("wait_for on a reached value after stop() returned true");
    }
    // stopped wins over a value reached before the stop; advance() does not revive it
    {
        Progress pr;
        for (int i = 0; i < 3; i++) pr.advance();
        if (!pr.wait_for(3)) return fail("wait_for(3) after three advances");
        pr.stop();
        if (pr.wait_for(3)) return fail("stopped does not win over a reached value");
        pr.advance();
        if (pr.wait_for(1)) return fail("advance() after stop() revived the counter");
    }
    // need <= 0 returns at once on a fresh counter
    {
        Progress pr;
        if (!pr.wait_for(0) || !pr.wait_for(-3)) return fail("wait_for(0) on a fresh counter");
    }
    printf("ok\n");
    return 0;
}
