// irec_call.h -- what the entry points of every container unit share (irec_rec*.hip, irec_res*.hip, irec_quality.hip, irec_rows.hip,
// irec_io.cpp): the calling thread's error text, the check of a launch, the check of a caller's workspace, and [0, n) dealt to host
// threads.  Host code only, no HIP header: IREC_HIP expands where it is used, in a unit that has one.
#ifndef IREC_CALL_H_
#define IREC_CALL_H_
#include <cstddef>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "irec.h"

namespace irec {
irec_status set_last_error(irec_status code, const char *who, const char *what);   // irec_host.cpp

// IREC_OK, or IREC_E_WORKSPACE under the entry's name: what a device entry says of a workspace that is null, not 8-byte aligned or
// smaller than need_bytes (sizer_name: the function of include/irec.h that tells the caller how much to bring)
inline irec_status check_workspace(size_t need_bytes, const void *workspace, size_t workspace_bytes, const char *who, const char *sizer_name) {
  if (workspace && !((uintptr_t)workspace & 7) && workspace_bytes >= need_bytes) return IREC_OK;
  return set_last_error(IREC_E_WORKSPACE, who, (std::string("workspace too small (") + sizer_name + ") or not 8-byte aligned").c_str());
}

// the host threads of a call that asks for n_threads: 0 = one per core, at most 32
inline int64_t host_threads(int32_t n_threads) {
  const int64_t T = n_threads > 0 ? n_threads : (int64_t)std::thread::hardware_concurrency();
  return T < 1 ? 1 : (T > 32 ? 32 : T);
}

// [0, n) dealt to host_threads(n_threads) threads in contiguous ranges, body(lo, hi) once per thread; no more threads than n / grain
// (a thread is not worth fewer than `grain` elements), and with one thread or none body(0, n) runs on the calling thread.  body must
// not throw: an exception that leaves a thread ends the process.
template <class F>
void parallel_chunks(int64_t n, int32_t n_threads, int64_t grain, F &&body) {
  int64_t T = host_threads(n_threads);
  if (T > n / grain) T = n / grain;
  if (T <= 1) { body((int64_t)0, n); return; }
  std::vector<std::thread> pool;
  for (int64_t t = 0; t < T; ++t) pool.emplace_back([&body, t, T, n]() { body(n * t / T, n * (t + 1) / T); });
  for (auto &th : pool) th.join();
}
// the same as the par(n, body) that the core headers' call forms take (irec_res_core.h, irec_res_fit_core.h, irec_quality_core.h)
struct Chunks {
  int32_t n_threads; int64_t grain;
  template <class F> void operator()(int64_t n, F &&body) const { parallel_chunks(n, n_threads, grain, body); }
};
} // namespace irec

// a HIP call or, after a launch, hipGetLastError(): on failure the entry returns IREC_E_HIP under `what` (IREC_HIP: the expression)
#define IREC_HIP_AS(what, expr)                                                                         \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return irec::set_last_error(IREC_E_HIP, what, hipGetErrorString(e_));          \
  } while (0)
#define IREC_HIP(expr) IREC_HIP_AS(#expr, expr)

#endif // IREC_CALL_H_
