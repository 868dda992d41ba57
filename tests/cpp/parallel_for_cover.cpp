// Host-side cover of csrc/host_common.h's parallel_for: the split of a per-item loop into parts for the worker pool.
// tests/test_parallel_for_ref.py replaces the marked line below with the header's own text, from `class WorkerPool {` to the end
// of parallel_for, and builds the result with g++ (no GPU, no HIP) — once plainly, once with -fsanitize=thread.
// MI355_SW_POOL_THREADS is read once per process, so the test starts one process per value.
// usage: parallel_for_cover [n ...]         every n (default: the list below) under the default threshold and inside a PoolFromScope;
//        parallel_for_cover --repeat R n ...  the same, R times over (the ThreadSanitizer run)
// One JSON object per (scope, n) and line on stdout; the test asserts on them.  Exit status 0 unless the harness itself failed.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// what the slice needs of the rest of the header: the two per-thread bindings of a call and the counter of pooled loops
struct Options { int tag = 0; };
struct DevInfo { int tag = 0; };
thread_local const Options *tl_opt = nullptr;
thread_local const DevInfo *tl_dev = nullptr;
thread_local size_t tl_pooled_loops = 0;

// @@HOST_COMMON_SLICE@@

namespace {

constexpr int kParts = 8;                                            // parts WorkerPool::run can execute (its own clamp)
Options worker_opt[kParts];                                          // what each pool thread holds as ITS OWN bindings (part t: worker t - 1)
DevInfo worker_dev[kParts];

// every pool thread takes bindings of its own (fix = true) / reports whether it still holds them (fix = false)
int workers_own(bool fix) {
  std::atomic<int> wrong{0};
  WorkerPool::get().run(kParts, [&](int t) {
    if (t == 0) return;
    if (fix) { tl_opt = &worker_opt[t]; tl_dev = &worker_dev[t]; }
    else if (tl_opt != &worker_opt[t] || tl_dev != &worker_dev[t]) wrong.fetch_add(1);
  });
  return wrong.load();
}

void one(const char *scope, size_t n) {
  const Options mine_opt; const DevInfo mine_dev;
  tl_opt = &mine_opt; tl_dev = &mine_dev;
  const std::thread::id caller = std::this_thread::get_id();
  std::vector<std::atomic<unsigned char>> hits(n + 1);              // (one spare entry: data() of an empty vector)
  for (auto &h : hits) h.store(0, std::memory_order_relaxed);
  std::atomic<long> calls{0}, off_caller{0}, bad_range{0}, wrong_binding{0};
  const size_t pooled_before = tl_pooled_loops;
  parallel_for(n, [&](size_t k0, size_t k1) {
    calls.fetch_add(1);
    if (std::this_thread::get_id() != caller) off_caller.fetch_add(1);
    if (tl_opt != &mine_opt || tl_dev != &mine_dev) wrong_binding.fetch_add(1);
    if (k0 > k1 || k1 > n) { bad_range.fetch_add(1); return; }
    for (size_t k = k0; k < k1; ++k) {
      const unsigned char was = hits[k].load(std::memory_order_relaxed);
      hits[k].store((unsigned char)std::min(250, was + 1), std::memory_order_relaxed);   // (a part owns its items: plain read-modify-write, a race if two parts share one)
    }
  });
  const size_t pooled = tl_pooled_loops - pooled_before;
  const bool caller_kept = tl_opt == &mine_opt && tl_dev == &mine_dev;
  size_t missed = 0, twice = 0, first_missed = n;
  for (size_t k = 0; k < n; ++k) {
    const unsigned char h = hits[k].load(std::memory_order_relaxed);
    if (h == 0) { if (!missed) first_missed = k; ++missed; }
    if (h > 1) ++twice;
  }
  const int restore_wrong = workers_own(false);
  printf("{\"scope\": \"%s\", \"pool_from\": %zu, \"n\": %zu, \"calls\": %ld, \"off_caller\": %ld, \"bad_range\": %ld, \"wrong_binding\": %ld, "
         "\"caller_kept\": %d, \"restore_wrong\": %d, \"missed\": %zu, \"first_missed\": %zu, \"twice\": %zu, \"pooled_loops\": %zu}\n",
         scope, tl_pool_from, n, calls.load(), off_caller.load(), bad_range.load(), wrong_binding.load(), (int)caller_kept, restore_wrong,
         missed, first_missed, twice, pooled);
  tl_opt = nullptr; tl_dev = nullptr;
}

}  // namespace

int main(int argc, char **argv) {
  std::vector<size_t> ns;
  int repeat = 1, a = 1;
  if (argc > 2 && !strcmp(argv[1], "--repeat")) { repeat = atoi(argv[2]); a = 3; }
  for (; a < argc; ++a) ns.push_back((size_t)strtoull(argv[a], nullptr, 10));
  if (ns.empty()) ns = {0, 1, 1023, 1024, 1025, 8191, 49151, 49152, 49153, 131071, 131072, 200003};
  if (WorkerPool::kMaxParts != kParts) { fprintf(stderr, "WorkerPool::kMaxParts is %d, this harness assumes %d\n", (int)WorkerPool::kMaxParts, kParts); return 2; }
  if (workers_own(true) != 0) return 2;
  for (int r = 0; r < repeat; ++r)
    for (size_t n : ns) {
      one("default", n);
      { PoolFromScope scope_; one("scoped", n); }
    }
  if (tl_pool_from != 131072) { fprintf(stderr, "PoolFromScope did not restore the threshold\n"); return 2; }
  fflush(stdout);
  return 0;
}
