// prt_tlas_worker.h -- the context's worker thread for the instance BVH's per-update builds (host only, no HIP).
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <ctime>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bvh_build.h"
#include "prt_refit.h"

namespace prt::host {

// The instance BVH's per-update build (ensure_instances) on the context's worker thread: each update's job builds
// the tree over that update's instance boxes into the update's pinned staging buffer, then sets the update's flag
// word; the render stream waits for the flag in a one-lane kernel (launch_wait_host) placed before the tree's
// upload, so the calling thread never builds nor waits, and the frames already queued run while the worker builds.
// (A host function, hipLaunchHostFunc, made the next enqueue on the stream block the calling thread until it had
// run: 5-11 ms per update with frames queued, scripts/inst_update_probe.py.)  Jobs run in submission order and every
// job sets its flag, also when its build fails; the worker never calls HIP.
struct TlasJob {
  const InstSrc* src = nullptr;  // the update's instances (in its pinned staging buffer, uploaded before the tree)
  int32_t n = 0;
  char* dst = nullptr;           // pinned: cap Node8 records, then 8 * cap slot words
  size_t cap = 0;                // nodes the upload moves (a tree over n instances has at most max(n, 1) nodes)
  int max_depth = 0;             // levels the traversal stacks were sized for (build_tlas8's cap)
  uint32_t* flag = nullptr;      // coherent pinned word: set to 1 once dst holds the tree
};
class TlasWorker {
 public:
  TlasWorker() : th_([this] { run(); }) {}
  ~TlasWorker() {  // after the streams are synchronised: the queue is empty (every job's stream wait has ended)
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  void seed(const BuiltTlas8& t) {  // the tree a failed build falls back to (its instance set's first tree)
    std::lock_guard<std::mutex> g(m_);
    good_nodes_ = t.nodes;
    good_slot_ = t.slot;
  }
  void submit(const std::shared_ptr<TlasJob>& j) {
    {
      std::lock_guard<std::mutex> g(m_);
      q_.push_back(j);
    }
    cv_.notify_all();
  }
  // prt_update_instances refits the tree the device holds: wait until every submitted job has finished (a host
  // condition variable: no GPU involved, bounded by the queued builds), then copy that tree out -- the last good one,
  // which is what the last job left in its update's staging buffer
  void wait_idle() {
    std::unique_lock<std::mutex> g(m_);
    idle_cv_.wait(g, [&] { return q_.empty() && !busy_; });
  }
  void last_tree(std::vector<Node8>& nodes, std::vector<uint32_t>& slot) {
    std::lock_guard<std::mutex> g(m_);
    nodes = good_nodes_;
    slot = good_slot_;
  }
  size_t last_tree_nodes() {
    std::lock_guard<std::mutex> g(m_);
    return good_nodes_.size();
  }
  // diagnostics of the finished jobs
  struct Stats { double ms = 0, cpu_ms = 0; int32_t median = 0, failed = 0; std::string err; };
  Stats stats() {
    std::lock_guard<std::mutex> g(m_);
    return st_;
  }

 private:
  void run() {
    for (;;) {
      std::shared_ptr<TlasJob> j;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;  // stop_ with nothing queued
        j = q_.front();
        q_.pop_front();
        busy_ = true;
      }
      const auto t0 = std::chrono::steady_clock::now();
      timespec c0{}, c1{};
      clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c0);
      bool median = false, ok = false;
      std::string err;
      BuiltTlas8 t;
      try {  // the instances' world boxes (the same refit_instance as k_refit), the SAH build over them
        const int32_t m = j->n;
        std::vector<float> boxes(6 * (size_t)m);
        for (int32_t i = 0; i < m; i++) {
          InstDev I;
          refit_instance(j->src[i], I);
          std::memcpy(&boxes[6 * (size_t)i], I.bmin, 12);
          std::memcpy(&boxes[6 * (size_t)i + 3], I.bmax, 12);
        }
        t = build_tlas8(boxes.data(), m, j->max_depth);
        median = t.median;
        ok = t.nodes.size() <= j->cap && t.depth <= j->max_depth;
        if (!ok) err = "instance BVH larger than planned";
      } catch (const std::exception& e) {
        err = e.what();
      }
      std::lock_guard<std::mutex> g(m_);
      const std::vector<Node8>& nodes = ok ? t.nodes : good_nodes_;  // failed: the last good tree (valid links)
      const std::vector<uint32_t>& slot = ok ? t.slot : good_slot_;
      std::memcpy(j->dst, nodes.data(), std::min(nodes.size(), j->cap) * sizeof(Node8));
      std::memcpy(j->dst + j->cap * sizeof(Node8), slot.data(), std::min(slot.size(), 8 * j->cap) * 4);
      if (ok) {
        good_nodes_ = std::move(t.nodes);
        good_slot_ = std::move(t.slot);
      } else {
        st_.failed++;
        st_.err = err;
      }
      clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c1);
      st_.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      st_.cpu_ms = (c1.tv_sec - c0.tv_sec) * 1e3 + (c1.tv_nsec - c0.tv_nsec) * 1e-6;
      st_.median += median ? 1 : 0;
      __atomic_store_n(j->flag, 1u, __ATOMIC_RELEASE);  // the tree is in dst: the stream's wait ends
      busy_ = false;
      idle_cv_.notify_all();
    }
  }
  std::mutex m_;
  std::condition_variable cv_, idle_cv_;
  std::deque<std::shared_ptr<TlasJob>> q_;
  bool stop_ = false, busy_ = false;  // busy_: a job was taken off the queue and has not finished
  std::vector<Node8> good_nodes_;
  std::vector<uint32_t> good_slot_;
  Stats st_;
  std::thread th_;  // last: started once the members above exist
};

}  // namespace prt::host
