// worker_pool.h — the host threads that the game groups (selfplay.cc) and the batching match driver (eval_match.cc) share.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace p3 {

// A pool of host threads that runs several ParallelFor jobs at once: every game group submits its
// own job from its own driver thread, the workers always take the oldest job that still has
// items, so a game that is slow to advance (a long ladder read-out) holds up its own group only.
class WorkerPool {
 public:
  explicit WorkerPool(int n) {
    for (int i = 0; i < n; ++i) threads_.emplace_back([this] { Loop(); });
  }
  ~WorkerPool() {
    {
      std::lock_guard<std::mutex> l(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
  struct Job {
    std::function<void(int)> fn;
    int total = 0, next = 0, unfinished = 0;   // guarded by the pool's mutex
    std::condition_variable done_cv;
  };
  using JobRef = std::shared_ptr<Job>;
  // runs fn(i) for i in [0, n) on the pool and returns when all are done; callable from several
  // threads at the same time
  template <class F>
  void ParallelFor(int n, F&& fn) {
    if (n <= 0) return;
    Wait(Submit(n, std::forward<F>(fn)));
  }
  // the same in two steps: the caller may stop waiting (WaitFor) and come back for the rest later (Wait); whatever
  // fn refers to must then live until that Wait returns
  template <class F>
  JobRef Submit(int n, F&& fn) {
    JobRef job = std::make_shared<Job>();
    job->fn = std::forward<F>(fn);
    job->total = n;
    job->unfinished = n;
    if (n > 0) {
      {
        std::lock_guard<std::mutex> l(mu_);
        jobs_.push_back(job);
      }
      cv_.notify_all();
    }
    return job;
  }
  void Wait(const JobRef& job) {
    std::unique_lock<std::mutex> l(mu_);
    job->done_cv.wait(l, [&] { return job->unfinished == 0; });
  }
  // waits at most `us` microseconds; the items not finished yet (0: done) and whether every item has been handed out.
  // (Polls under the mutex between short sleeps: no timed condition-variable wait, whose pthread_cond_clockwait the
  // ThreadSanitizer of this toolchain does not model.)
  int WaitFor(const JobRef& job, long us, bool* all_started) {
    const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(us);
    for (;;) {
      {
        std::lock_guard<std::mutex> l(mu_);
        if (job->unfinished == 0 || std::chrono::steady_clock::now() >= until) {
          if (all_started) *all_started = job->next == job->total;
          return job->unfinished;
        }
      }
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  }

 private:
  void Loop() {
    std::unique_lock<std::mutex> l(mu_);
    for (;;) {
      JobRef job;
      cv_.wait(l, [&] {
        if (stop_) return true;
        for (const JobRef& j : jobs_)
          if (j->next < j->total) { job = j; return true; }
        return false;
      });
      if (stop_) return;
      const int i = job->next++;
      if (job->next == job->total) jobs_.erase(std::find(jobs_.begin(), jobs_.end(), job));   // no items left to hand out
      l.unlock();
      job->fn(i);
      l.lock();
      if (--job->unfinished == 0) job->done_cv.notify_all();
    }
  }
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<JobRef> jobs_;   // oldest first
  bool stop_ = false;
};

}  // namespace p3
