// gm_once.h -- Once<T>: the one protocol by which a handle's lazily built structures are published.
// A value of type T (a struct of DevOwn arrays and the scalars that describe them, or a single fact about the graph) plus a state:
// unknown, built, or not applicable ("looked at, and this handle has none").
//   read    one acquire load.  A reader that sees built or not applicable may read T without the lock for the rest of the handle's life:
//           operator-> / operator* go through the state and hand out an EMPTY T while it is unknown, so a reader cannot reach a half-made
//           member, and "no such structure" reads as the defaults of T (null arrays, zero counts).
//   build   ensure(mu, builder): under `mu` (every caller passes the handle's own, which is not recursive -- prerequisites that take it
//           themselves are called before) the state is checked again and builder(T &local) fills a LOCAL value.  It returns kOnceBuilt,
//           kOnceNotApplicable or an error code of the library; only on the first two is the local moved in and the state stored, with
//           release order -- the one place a state is written.  On an error nothing is published, the state stays unknown (the next call
//           tries again) and what the builder had allocated goes back through the DevOwn members of the local.
//   reset   back to unknown and an empty T.  For gm_graph_sort_neighbors alone, which rewrites the rows and with them the two row-order
//           facts, on a handle no solver has used yet: no other thread may be reading.
// Needs nothing but the standard library: a plain host compiler builds it (tests/once_host_check.cc).
#pragma once
#include <atomic>
#include <mutex>
#include <utility>

constexpr int kOnceBuilt = 0;           // (== GM_OK: a builder that only ever builds may return the library's codes as they are)
constexpr int kOnceNotApplicable = -1;  // (no error code of the library is negative)

template <class T>
class Once {
  enum : int { kUnknown = 0, kBuilt = 1, kNotApplicable = 2 };
  T v_{};
  std::atomic<int> st_{kUnknown};
  const T &value() const {
    static const T none{};
    return st_.load(std::memory_order_acquire) != kUnknown ? v_ : none;
  }

 public:
  Once() = default;
  Once(const Once &) = delete;
  Once &operator=(const Once &) = delete;
  bool built() const { return st_.load(std::memory_order_acquire) == kBuilt; }
  bool known() const { return st_.load(std::memory_order_acquire) != kUnknown; }  // built or not applicable
  const T *operator->() const { return &value(); }
  const T &operator*() const { return value(); }
  // GM_OK (0) when the value is there or known not to apply -- before or after this call -- else the builder's error code
  template <class F>
  int ensure(std::mutex &mu, F &&builder) {
    if (known()) return 0;
    std::lock_guard<std::mutex> lk(mu);
    if (st_.load(std::memory_order_relaxed) != kUnknown) return 0;
    T local{};
    const int rc = builder(local);
    if (rc != kOnceBuilt && rc != kOnceNotApplicable) return rc;
    v_ = std::move(local);
    st_.store(rc == kOnceBuilt ? kBuilt : kNotApplicable, std::memory_order_release);
    return 0;
  }
  void reset() {  // (gm_graph_sort_neighbors only: see above)
    v_ = T{};
    st_.store(kUnknown, std::memory_order_release);
  }
};
