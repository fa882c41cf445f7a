// zw_progress.h -- the pipeline's cross-thread hand-shake: a monotone counter
// one thread advances and others wait on, with a terminal "stopped" value.
#pragma once
#include <condition_variable>
#include <limits>
#include <mutex>

class Progress {
public:
    // One more step is done.  (A stopped counter stays stopped.)
    void advance()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (v_ != kStopped) v_++;
        }
        cv_.notify_all();
    }
    // No further step will come: every present and later wait_for fails.
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            v_ = kStopped;
        }
        cv_.notify_all();
    }
    // Blocks until `need` steps are done (true) or the counter is stopped
    // (false: stopped wins, also over a value reached before the stop).
    bool wait_for(long long need)
    {
        if (need <= 0) return true;
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return v_ >= need; });
        return v_ != kStopped;
    }

private:
    static constexpr long long kStopped = std::numeric_limits<long long>::max();
    std::mutex mu_;
    std::condition_variable cv_;
    long long v_ = 0;
};
