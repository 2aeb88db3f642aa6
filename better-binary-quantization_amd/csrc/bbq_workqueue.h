// bbq_workqueue.h - persistent host threads behind one FIFO of jobs: the heap replays of the search path (a pool, never destroyed)
// and the per-shard worker of a multi-device index (one thread, joined with its shard).
#pragma once
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace bbq {

class WorkQueue {
 public:
  explicit WorkQueue(int n_threads = 0) { ensure(n_threads); }
  ~WorkQueue() {  // runs what is still queued, then joins the threads
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
    cv_.notify_all();
    for (std::thread &t : th_) t.join();
  }
  void ensure(int n) {  // at least n threads from here on
    std::lock_guard<std::mutex> lk(m_);
    while ((int)th_.size() < n) th_.emplace_back([this] { run(); });
  }
  void post(std::function<void()> f) {
    { std::lock_guard<std::mutex> lk(m_); q_.push_back(std::move(f)); }
    cv_.notify_one();
  }
 private:
  void run() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;
        f = std::move(q_.front());
        q_.pop_front();
      }
      f();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  bool stop_ = false;
  std::vector<std::thread> th_;
};

}  // namespace bbq
