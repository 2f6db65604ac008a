// body(i) for i in [0, n) on `threads` host threads (0: one per hardware thread), item i on thread
// i % threads.
#pragma once

#include <algorithm>
#include <thread>
#include <vector>

template <typename F>
void parallel_for(int n, int threads, F&& body) {
  if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
  threads = std::min(threads, std::max(1, n));
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t]() {
      for (int i = t; i < n; i += threads) body(i);
    });
  for (auto& th : pool) th.join();
}
