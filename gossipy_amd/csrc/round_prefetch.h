// Bounded producer/consumer for per-round work (plain C++, no pybind).
//
// A worker thread calls produce(r) for consecutive rounds r = first,
// first + 1, ... and keeps at most `depth` finished rounds waiting; the
// consumer collects them in order with take(r). An exception thrown by
// produce() ends the worker; take() hands out the rounds finished before it
// and then rethrows it. The destructor stops the worker (after the round it
// is producing, if any) and joins it.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

template <typename T>
class RoundPrefetch {
public:
    using Produce = std::function<T(int64_t)>;

    RoundPrefetch(Produce produce, int64_t first, size_t depth = 2)
        : produce_(std::move(produce)), depth_(depth), next_take_(first),
          next_prod_(first), worker_([this] { run(); })
    {
    }

    RoundPrefetch(const RoundPrefetch&) = delete;
    RoundPrefetch& operator=(const RoundPrefetch&) = delete;

    ~RoundPrefetch() { stop(); }

    // the round the next take() must ask for
    int64_t next() const
    {
        std::lock_guard<std::mutex> lk(m_);
        return next_take_;
    }

    // blocks until round r is ready; r must be next()
    T take(int64_t r)
    {
        std::unique_lock<std::mutex> lk(m_);
        if (r != next_take_)
            throw std::invalid_argument(
                "rounds are prefetched in order: expected round " +
                std::to_string(next_take_) + ", got " + std::to_string(r));
        ready_cv_.wait(lk, [&] { return !ready_.empty() || err_ || stop_; });
        if (ready_.empty()) {
            if (err_) std::rethrow_exception(err_);
            throw std::logic_error("take() on a stopped prefetcher");
        }
        T v = std::move(ready_.front());
        ready_.pop_front();
        ++next_take_;
        lk.unlock();
        space_cv_.notify_one();
        return v;
    }

    // stop the worker and hand back the finished rounds nobody took yet,
    // in order, the first one being round next(); afterwards the producer's
    // state stands right after the last round returned here
    std::vector<T> drain()
    {
        stop();
        std::vector<T> rest;
        for (auto& v : ready_) rest.push_back(std::move(v));
        ready_.clear();
        return rest;
    }

private:
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        space_cv_.notify_all();
        ready_cv_.notify_all();
        if (worker_.joinable()) worker_.join();
    }

    void run()
    {
        for (;;) {
            int64_t r;
            {
                std::unique_lock<std::mutex> lk(m_);
                space_cv_.wait(
                    lk, [&] { return stop_ || ready_.size() < depth_; });
                if (stop_) return;
                r = next_prod_;
            }
            try {
                T v = produce_(r);
                std::lock_guard<std::mutex> lk(m_);
                ready_.push_back(std::move(v));
                ++next_prod_;
            } catch (...) {
                std::lock_guard<std::mutex> lk(m_);
                err_ = std::current_exception();
                ready_cv_.notify_all();
                return;
            }
            ready_cv_.notify_all();
        }
    }

    Produce produce_;
    size_t depth_;
    mutable std::mutex m_;
    std::condition_variable ready_cv_, space_cv_;
    std::deque<T> ready_;
    int64_t next_take_, next_prod_;
    std::exception_ptr err_;
    bool stop_ = false;
    std::thread worker_;  // last: starts once everything above exists
};
