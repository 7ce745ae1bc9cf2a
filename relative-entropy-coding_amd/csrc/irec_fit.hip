// irec_fit.hip -- the fitter of the auxiliary-variance ratios: GaussianCoder.update_block_auxiliary_variance_ratios
// (rec/coding/coder.py:266-410) on the device (gfx950) and its host twin, bit for bit the same.
//
// Arithmetic contract: DESIGN.md §3 "ratio fit".  The statistics are float32; every operation of the fit itself is a correctly
// rounded float64 + - * / over det_log / det_exp (irec_device.h), no contraction; sums over the dims of a row and over the rows of a
// step take the canonical tree of block_kl_kernel (groups of 256, lane l chains 4l .. 4l+3, lanes paired at distance 32 .. 1, group
// sums added in order); the hand-over to the next ratio is float32 in the operator order of the sequential importance coder.
//
// Per fit step (ratio = M .. 2):
//   fit_rows_kernel      the selected rows' KL (tot) and the constants w = tv / cv - 1, s = u + w of every element
//   fit_iter_kernel      ONE SGD iteration per launch.  A workgroup sums rows (aux_kl, g), publishes them and draws a ticket; the
//                        workgroup that draws the last one reduces the rows, updates theta / prev / iters and sets `done`.  Every
//                        launch begins by reading `done` and leaves at once when it is set: the host enqueues launches in chunks
//                        (FIT_CHUNK) and reads `done` between chunks.  No workgroup ever waits for another.
//   fit_handover_kernel  coder.py:390-408: the auxiliary sample and the conditional target / coder, in place in the workspace
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <exception>
#include <thread>
#include <vector>

#include "irec_call.h"
#include "irec_device.h"
#include "irec_internal.h"
#include "irec_kernels.h"

namespace irec {

namespace {

constexpr int FIT_NT = 256;
constexpr int FIT_CHUNK = 64;             // launches between two reads of `done`
std::atomic<int> g_fit_chunk{FIT_CHUNK};

struct FitState {
  double theta, prev, rho_last, loss;
  int32_t iters, done;
  uint32_t ticket;
  int32_t pad;
};

struct FitLayout {
  size_t stats[4], W, S, tot, pair, sel, num, kl, state, bytes;
};
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
FitLayout fit_layout(int64_t n, int32_t D) {
  FitLayout L;
  const size_t E = (size_t)n * (size_t)D;
  size_t at = 0;
  for (int i = 0; i < 4; ++i) { L.stats[i] = at; at += up256(E * 4); }
  L.W = at; at += up256(E * 8);
  L.S = at; at += up256(E * 8);
  L.tot = at; at += up256((size_t)n * 8);
  L.pair = at; at += up256((size_t)n * 16);
  L.sel = at; at += up256((size_t)n * 4);
  L.num = at; at += up256((size_t)n * 4);
  L.kl = at; at += up256((size_t)n * 4);
  L.state = at; at += 256;
  L.bytes = at;
  return L;
}

// num_aux_variables = 1 + floor(total_kl / Omega) in float32 (coder.py:284)
__host__ __device__ inline int32_t fit_num(float kl, float omega) {
  const float k = __builtin_floorf(kl / omega);
  if (!(k == k)) return 0;
  if (!(k < 1.0e9f)) return 1000000000;
  if (k < -1.0f) return 0;
  return 1 + (int32_t)k;
}

// the loss and gradient terms of one row (coder.py:360-367 and their derivative w.r.t. the ratio)
__host__ __device__ inline void fit_row_terms(double aux_kl, double g, double tot, double om, double om_rest, double &l, double &gt) {
  const double e1 = aux_kl - om;
  const double e2 = (tot - aux_kl) - om_rest;
  const double l1 = e1 > 0.0 ? e1 * e1 : 0.0, l2 = e2 > 0.0 ? e2 * e2 : 0.0;
  const double g1 = e1 > 0.0 ? (2.0 * e1) * g : 0.0, g2 = e2 > 0.0 ? (2.0 * e2) * g : 0.0;
  l = l1 + l2;
  gt = g1 - g2;
}

// the update of one iteration (coder.py:369-376); returns true when the step is over
__host__ __device__ inline bool fit_update(FitState &st, double rho, double sumL, double sumG, int ns, double lr, double tol, int max_iters) {
  const double L = sumL / (double)ns;
  const double G = (sumG / (double)ns) * (rho * (1.0 - rho));
  st.theta = st.theta - lr * G;
  st.rho_last = rho;
  st.loss = L;
  st.iters += 1;
  const double diff = st.prev - L;
  const double ad = diff < 0.0 ? -diff : diff;
  bool over = ad < tol;
  if (!over) st.prev = L;
  if (st.iters >= max_iters) over = true;
  return over;
}

// the hand-over of one element (coder.py:385-408; formulas of the sequential importance coder, float32)
__host__ __device__ inline void fit_handover(float &mq, float &sq, float &mp, float &sp, float r_last, float r_avg, float x) {
  const float cv = sp * sp, tv = sq * sq;
  const float al = r_last * cv;
  const float ta_loc = (mq - mp) * al / cv;
  const float ta_scale = __builtin_sqrtf(tv * (al * al) / (cv * cv) + al * (cv - al) / cv);
  const float A = ta_loc + ta_scale * x;
  const float a = r_avg * cv;
  const float nmq = mp + (A * tv * cv + (mq - mp) * (cv - a) * cv) / (tv * a + cv * (cv - a));
  const float nsq = __builtin_sqrtf(tv * cv * (cv - a) / (a * tv + cv * (cv - a)));
  const float nmp = mp + A;
  const float nsp = __builtin_sqrtf(cv - a);
  mq = nmq; sq = nsq; mp = nmp; sp = nsp;
}

__host__ __device__ inline void fit_consts(float mq, float sq, float mp, float sp, double &w, double &s) {
  const double cv = (double)sp * (double)sp, tv = (double)sq * (double)sq;
  const double dm = (double)mq - (double)mp;
  const double u = (dm * dm) / cv;
  w = tv / cv - 1.0;
  s = u + w;
}

// ---- the canonical tree on the host: f(i) for i < count -------------------------------------------------------------------
template <class F>
double host_tree(int64_t count, F f) {
  double total = 0.0;
  const int64_t NG = (count + 255) >> 8;
  for (int64_t g = 0; g < NG; ++g) {
    double lanes[64], nxt[64];
    for (int l = 0; l < 64; ++l) {
      double acc = 0.0;
      for (int i = 0; i < 4; ++i) {
        const int64_t d = g * 256 + l * 4 + i;
        if (d < count) acc = acc + f(d);
      }
      lanes[l] = acc;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      for (int l = 0; l < 64; ++l) nxt[l] = lanes[l] + lanes[l ^ off];
      std::memcpy(lanes, nxt, sizeof(lanes));
    }
    total = g == 0 ? lanes[0] : total + lanes[0];
  }
  return total;
}

template <class F>
void host_rows(int64_t n, int n_threads, int64_t work_per_row, F f) {
  int nt = n_threads > 0 ? n_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  nt = (int)std::min<int64_t>(std::min(nt, 16), n);
  if (n * work_per_row < 32768) nt = 1;
  if (nt <= 1) {
    for (int64_t k = 0; k < n; ++k) f(k);
    return;
  }
  std::atomic<int64_t> next{0};
  auto work = [&]() { for (int64_t k = next.fetch_add(1); k < n; k = next.fetch_add(1)) f(k); };
  std::vector<std::thread> pool;
  pool.reserve((size_t)nt);
  try {
    for (int i = 1; i < nt; ++i) pool.emplace_back(work);
  } catch (const std::exception &) {}
  work();
  for (auto &t : pool) t.join();
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
struct FitRowsArgs {
  const float *mq, *sq, *mp, *sp;    // [n_rows, D]
  const int32_t *sel;                // selected rows (NULL: row k = k)
  int32_t n_sel, D;
  double *tot; float *kl; int32_t *num; float omega;   // kl / num: NULL for a fit step
  double *W, *S;                     // constants [n_sel, D] (NULL: none)
  FitState *state; double theta0;    // initialised by workgroup 0 (NULL: not)
};

// two canonical sums at once over the dims of one row; all threads return with the totals of (a, b)
template <class F>
__device__ __forceinline__ void fit_tree2(int D, F f, double &ta, double &tb, double (*gpart)[2], double *total_s) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NG = (D + 255) >> 8;
  for (int g0 = 0; g0 < NG; g0 += 4) {
    const int g = g0 + wave;
    double a = 0.0, b = 0.0;
    if (g < NG) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = g * 256 + lane * 4 + i;
        if (d < D) {
          double va, vb;
          f(d, va, vb);
          a = a + va;
          b = b + vb;
        }
      }
    }
    const double sa = wave_tree_sum(a), sb = wave_tree_sum(b);
    if (lane == 0) { gpart[wave][0] = sa; gpart[wave][1] = sb; }
    __syncthreads();
    if (tid == 0) {
      double t0 = g0 == 0 ? 0.0 : total_s[0], t1 = g0 == 0 ? 0.0 : total_s[1];
      for (int w = 0; w < 4 && g0 + w < NG; ++w) {
        t0 = (g0 + w == 0) ? gpart[w][0] : t0 + gpart[w][0];
        t1 = (g0 + w == 0) ? gpart[w][1] : t1 + gpart[w][1];
      }
      total_s[0] = t0; total_s[1] = t1;
    }
    __syncthreads();
  }
  ta = NG ? total_s[0] : 0.0;
  tb = NG ? total_s[1] : 0.0;
  __syncthreads();   // (total_s is rewritten by the next row)
}

__global__ __launch_bounds__(FIT_NT) void fit_rows_kernel(FitRowsArgs A) {
  __shared__ double gpart[4][2];
  __shared__ double total_s[2];
  if (A.state && blockIdx.x == 0 && threadIdx.x == 0) {
    FitState st;
    st.theta = A.theta0; st.prev = __builtin_bit_cast(double, (uint64_t)0x7FF0000000000000ull); st.rho_last = 0.0; st.loss = 0.0;
    st.iters = 0; st.done = 0; st.ticket = 0u; st.pad = 0;
    *A.state = st;
  }
  for (int k = blockIdx.x; k < A.n_sel; k += gridDim.x) {
    const int64_t row = A.sel ? A.sel[k] : k;
    const float *mq = A.mq + row * A.D, *sq = A.sq + row * A.D, *mp = A.mp + row * A.D, *sp = A.sp + row * A.D;
    double *W = A.W ? A.W + (int64_t)k * A.D : nullptr, *S = A.S ? A.S + (int64_t)k * A.D : nullptr;
    double t, unused;
    fit_tree2(A.D, [&](int d, double &va, double &vb) {
      va = kl_dim(mq[d], sq[d], mp[d], sp[d]);
      vb = 0.0;
      if (W) {
        double w, s;
        fit_consts(mq[d], sq[d], mp[d], sp[d], w, s);
        W[d] = w; S[d] = s;
      }
    }, t, unused, gpart, total_s);
    if (threadIdx.x == 0) {
      A.tot[k] = t;
      if (A.kl) { const float kl = (float)t; A.kl[k] = kl; A.num[k] = fit_num(kl, A.omega); }
    }
  }
}

struct FitIterArgs {
  FitState *state; const double *W, *S, *tot; double *pair;
  int32_t n_sel, D, max_iters;
  double om, om_rest, lr, tol;
};

__device__ __forceinline__ double fit_load_agent(const double *p) {
  return __builtin_bit_cast(double, __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void fit_store_agent(double *p, double v) {
  __hip_atomic_store((unsigned long long *)p, __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FIT_NT) void fit_iter_kernel(FitIterArgs A) {
  __shared__ double gpart[4][2];
  __shared__ double total_s[2];
  __shared__ int s_last;
  // (state is written only by the workgroup that draws the LAST ticket of a launch, i.e. after every workgroup has read it here)
  if (A.state->done) return;
  const double theta = A.state->theta;
  const double rho = 1.0 / (1.0 + det_exp(-theta));
  const int tid = threadIdx.x;
  for (int k = blockIdx.x; k < A.n_sel; k += gridDim.x) {
    const double *W = A.W + (int64_t)k * A.D, *S = A.S + (int64_t)k * A.D;
    double aux_kl, g;
    fit_tree2(A.D, [&](int d, double &va, double &vb) {
      const double w = W[d], s = S[d];
      const double t = 1.0 + rho * w;
      va = 0.5 * (rho * s - det_log(t));
      vb = 0.5 * (s - w / t);
    }, aux_kl, g, gpart, total_s);
    if (tid == 0) { fit_store_agent(A.pair + 2 * k, aux_kl); fit_store_agent(A.pair + 2 * k + 1, g); }
  }
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t ticket = __hip_atomic_fetch_add(&A.state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == gridDim.x - 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last || tid >= 64) return;
  // the last arriver's first wave: rows in the canonical tree over the selection index
  const int lane = tid;
  double sumL = 0.0, sumG = 0.0;
  const int NG = (A.n_sel + 255) >> 8;
  for (int gI = 0; gI < NG; ++gI) {
    double aL = 0.0, aG = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = gI * 256 + lane * 4 + i;
      if (k < A.n_sel) {
        double l, gt;
        fit_row_terms(fit_load_agent(A.pair + 2 * k), fit_load_agent(A.pair + 2 * k + 1), A.tot[k], A.om, A.om_rest, l, gt);
        aL = aL + l;
        aG = aG + gt;
      }
    }
    const double sL = wave_tree_sum(aL), sG = wave_tree_sum(aG);
    sumL = gI == 0 ? sL : sumL + sL;
    sumG = gI == 0 ? sG : sumG + sG;
  }
  if (lane == 0) {
    FitState st = *A.state;
    st.theta = theta;
    const bool over = fit_update(st, rho, sumL, sumG, A.n_sel, A.lr, A.tol, A.max_iters);
    st.done = over ? 1 : 0;
    st.ticket = 0u;
    *A.state = st;
  }
}

struct FitHandArgs {
  float *mq, *sq, *mp, *sp; const int32_t *sel; const float *tab;   // tab: the step's table, [D][S_pad]
  int32_t n_sel, D, S_pad; float r_last, r_avg;
};

__global__ __launch_bounds__(FIT_NT) void fit_handover_kernel(FitHandArgs A) {
  const int64_t n = (int64_t)A.n_sel * A.D;
  for (int64_t e = (int64_t)blockIdx.x * FIT_NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * FIT_NT) {
    const int k = (int)(e / A.D), d = (int)(e % A.D);
    const int64_t row = A.sel[k], ix = row * A.D + d;
    float mq = A.mq[ix], sq = A.sq[ix], mp = A.mp[ix], sp = A.sp[ix];
    fit_handover(mq, sq, mp, sp, A.r_last, A.r_avg, A.tab[(size_t)d * (size_t)A.S_pad + (size_t)row]);
    A.mq[ix] = mq; A.sq[ix] = sq; A.mp[ix] = mp; A.sp[ix] = sp;
  }
}

// ---- what host twin and device driver share --------------------------------------------------------------------------------
const char *fit_check(const irec_fit_params *p, int64_t n_rows, int32_t dim) {
  if (!p) return "null parameters";
  if (!(p->kl_per_partition > 0.0f)) return "kl_per_partition must be positive";
  if (!(p->relative_tolerance == p->relative_tolerance) || !(p->learning_rate == p->learning_rate)) return "NaN parameter";
  if (p->max_iters < 1) return "max_iters must be at least 1";
  if (n_rows < 1 || n_rows > (1 << 24)) return "n_rows outside [1, 2^24]";
  if (dim < 1) return "dim must be positive";
  if ((size_t)n_rows * (size_t)dim > ((size_t)1 << 31)) return "more than 2^31 elements";
  return nullptr;
}

// num[] checked, M; NULL on success
const char *fit_counts(const float *kl, const int32_t *num, int64_t n, int32_t *M) {
  int32_t m = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(kl[i])) return "a row's KL divergence is infinite or NaN";
    m = std::max(m, num[i]);
  }
  if (m > IREC_MAX_PARTITIONS) return "a row needs more than IREC_MAX_PARTITIONS partitions";
  *M = m;
  return nullptr;
}

// the start value of a fit step: coder.py:324-331 (sigmoid_inverse, clip included, in float64 over det_log)
double fit_theta0(const float *ratios, int32_t ratio, int32_t M) {
  float init;
  if (ratios[ratio - 1] > 0.0f) init = ratios[ratio - 1];
  else if (ratio < M) init = ratios[ratio];
  else init = 1.0f / (float)ratio;
  double x = (double)init;
  if (x < 1e-10) x = 1e-10;
  if (x > 1.0 - 1e-10) x = 1.0 - 1e-10;
  return det_log(x) - det_log(1.0 - x);
}

// coder.py:385-389 in float32; returns the averaged ratio
float fit_average(float *ratios, float *counts, int32_t ratio, float r_last, int32_t ns) {
  const float c = counts[ratio - 1], nf = (float)ns;
  const float avg = (ratios[ratio - 1] * c + r_last * nf) / (c + nf);
  ratios[ratio - 1] = avg;
  counts[ratio - 1] = c + nf;
  return avg;
}

} // namespace

hipError_t launch_fit_rows(const FitRowsArgs &A, int grid, hipStream_t st) {
  hipLaunchKernelGGL(fit_rows_kernel, dim3(grid), dim3(FIT_NT), 0, st, A);
  return hipGetLastError();
}

} // namespace irec

// ================================================================================================================================
//  C ABI
// ================================================================================================================================
// (irec_host.cpp: the calling thread's irec_last_error text, and what the launches need to know of a context)
namespace irec { int context_device(const irec_context *ctx); int context_cus(const irec_context *ctx); }

extern "C" {

int32_t irec_test_fit_chunk(int32_t chunk) {
  return irec::g_fit_chunk.exchange(chunk > 0 ? chunk : irec::FIT_CHUNK);
}

irec_status irec_test_det_exp(const double *in, int64_t n, double *out) {
  if (n < 0 || (n > 0 && (!in || !out))) return irec::set_last_error(IREC_E_INVALID, "irec_test_det_exp", "bad arguments");
  for (int64_t i = 0; i < n; ++i) out[i] = irec::det_exp(in[i]);
  return IREC_OK;
}

size_t irec_fit_workspace_bytes(int64_t n_rows, int32_t dim) {
  if (n_rows < 1 || dim < 1 || n_rows > (1 << 24) || (size_t)n_rows * (size_t)dim > ((size_t)1 << 31)) return 0;
  return irec::fit_layout(n_rows, dim).bytes;
}

irec_status irec_fit_partitions_host(float kl_per_partition, int64_t n_rows, int32_t dim, const float *q_loc, const float *q_scale,
                                     const float *p_loc, const float *p_scale, float *out_kl, int32_t *out_num, int32_t n_threads) try {
  using namespace irec;
  irec_fit_params P{kl_per_partition, 0.0, 0.0, 1};
  if (const char *why = fit_check(&P, n_rows, dim)) return set_last_error(IREC_E_INVALID, "irec_fit_partitions_host", why);
  if (!q_loc || !q_scale || !p_loc || !p_scale || !out_kl || !out_num)
    return set_last_error(IREC_E_INVALID, "irec_fit_partitions_host", "null pointer argument");
  host_rows(n_rows, n_threads, dim, [&](int64_t k) {
    const float *mq = q_loc + k * dim, *sq = q_scale + k * dim, *mp = p_loc + k * dim, *sp = p_scale + k * dim;
    const float kl = (float)host_tree(dim, [&](int64_t d) { return kl_dim(mq[d], sq[d], mp[d], sp[d]); });
    out_kl[k] = kl;
    out_num[k] = fit_num(kl, kl_per_partition);
  });
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_fit_partitions_host", e.what()); }

irec_status irec_fit_aux_ratios_host(const irec_fit_params *p, int64_t n_rows, int32_t dim, const float *q_loc, const float *q_scale,
                                     const float *p_loc, const float *p_scale, const float *normal_table, int32_t table_steps,
                                     float *ratios, float *average_counts, int32_t capacity, int32_t *length, int32_t *out_iters,
                                     void *workspace, size_t workspace_bytes, int32_t n_threads) try {
  using namespace irec;
  const char *who = "irec_fit_aux_ratios_host";
  if (const char *why = fit_check(p, n_rows, dim)) return set_last_error(IREC_E_INVALID, who, why);
  if (!q_loc || !q_scale || !p_loc || !p_scale || !ratios || !average_counts || !length || !workspace)
    return set_last_error(IREC_E_INVALID, who, "null pointer argument");
  if (*length < 1 || *length > capacity) return set_last_error(IREC_E_INVALID, who, "length outside [1, capacity]");
  const FitLayout L = fit_layout(n_rows, dim);
  if (workspace_bytes < L.bytes) return set_last_error(IREC_E_WORKSPACE, who, "workspace smaller than irec_fit_workspace_bytes()");
  char *ws = (char *)workspace;
  const int64_t n = n_rows, D = dim;
  const size_t E = (size_t)n * (size_t)D;
  float *mq = (float *)(ws + L.stats[0]), *sq = (float *)(ws + L.stats[1]), *mp = (float *)(ws + L.stats[2]), *sp = (float *)(ws + L.stats[3]);
  std::memcpy(mq, q_loc, E * 4); std::memcpy(sq, q_scale, E * 4); std::memcpy(mp, p_loc, E * 4); std::memcpy(sp, p_scale, E * 4);
  double *W = (double *)(ws + L.W), *S = (double *)(ws + L.S), *tot = (double *)(ws + L.tot), *pair = (double *)(ws + L.pair);
  int32_t *sel = (int32_t *)(ws + L.sel), *num = (int32_t *)(ws + L.num);
  float *kl = (float *)(ws + L.kl);
  if (irec_status s = irec_fit_partitions_host(p->kl_per_partition, n_rows, dim, q_loc, q_scale, p_loc, p_scale, kl, num, n_threads)) return s;
  int32_t M = 0;
  if (const char *why = fit_counts(kl, num, n, &M)) return set_last_error(IREC_E_INVALID, who, why);
  const int32_t cur = *length;
  if (std::max(M, cur) > capacity) return set_last_error(IREC_E_INVALID, who, "capacity smaller than the partitions the rows need");
  if (M > 1 && (!normal_table || table_steps < M - 1 || !out_iters)) return set_last_error(IREC_E_INVALID, who, "the normal table covers fewer than M - 1 steps");
  for (int32_t i = cur; i < M; ++i) { ratios[i] = 0.0f; average_counts[i] = 0.0f; }   // coder.py:289-302
  *length = std::max(M, cur);
  const size_t S_pad = ((size_t)n + IREC_NORMAL_TABLE_PAD - 1) / IREC_NORMAL_TABLE_PAD * IREC_NORMAL_TABLE_PAD;
  const double om = (double)p->kl_per_partition;
  for (int32_t ratio = M; ratio >= 2; --ratio) {
    const int32_t j = M - ratio;
    int32_t ns = 0;
    for (int64_t i = 0; i < n; ++i) if (num[i] >= ratio) sel[ns++] = (int32_t)i;
    host_rows(ns, n_threads, D, [&](int64_t k) {
      const size_t r0 = (size_t)sel[k] * (size_t)D;
      double *Wk = W + (size_t)k * D, *Sk = S + (size_t)k * D;
      tot[k] = host_tree(D, [&](int64_t d) { return kl_dim(mq[r0 + d], sq[r0 + d], mp[r0 + d], sp[r0 + d]); });
      for (int64_t d = 0; d < D; ++d) fit_consts(mq[r0 + d], sq[r0 + d], mp[r0 + d], sp[r0 + d], Wk[d], Sk[d]);
    });
    FitState st{};
    st.theta = fit_theta0(ratios, ratio, M);
    st.prev = INFINITY;
    const double om_rest = om * (double)(ratio - 1);
    for (;;) {
      const double rho = 1.0 / (1.0 + det_exp(-st.theta));
      host_rows(ns, n_threads, D, [&](int64_t k) {
        const double *Wk = W + (size_t)k * D, *Sk = S + (size_t)k * D;
        pair[2 * k] = host_tree(D, [&](int64_t d) { const double t = 1.0 + rho * Wk[d]; return 0.5 * (rho * Sk[d] - det_log(t)); });
        pair[2 * k + 1] = host_tree(D, [&](int64_t d) { const double t = 1.0 + rho * Wk[d]; return 0.5 * (Sk[d] - Wk[d] / t); });
      });
      const double sumL = host_tree(ns, [&](int64_t k) { double l, gt; fit_row_terms(pair[2 * k], pair[2 * k + 1], tot[k], om, om_rest, l, gt); return l; });
      const double sumG = host_tree(ns, [&](int64_t k) { double l, gt; fit_row_terms(pair[2 * k], pair[2 * k + 1], tot[k], om, om_rest, l, gt); return gt; });
      if (fit_update(st, rho, sumL, sumG, ns, p->learning_rate, p->relative_tolerance, p->max_iters)) break;
    }
    out_iters[j] = st.iters;
    const float r_last = (float)st.rho_last;
    const float r_avg = fit_average(ratios, average_counts, ratio, r_last, ns);
    const float *tab = normal_table + (size_t)j * (size_t)D * S_pad;
    host_rows(ns, n_threads, D, [&](int64_t k) {
      const size_t row = (size_t)sel[k], r0 = row * (size_t)D;
      for (int64_t d = 0; d < D; ++d) fit_handover(mq[r0 + d], sq[r0 + d], mp[r0 + d], sp[r0 + d], r_last, r_avg, tab[(size_t)d * S_pad + row]);
    });
  }
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_fit_aux_ratios_host", e.what()); }

// the counts of every row on the device (out_kl / out_num: HOST memory; synchronises the stream)
irec_status irec_fit_partitions(irec_context *ctx, float kl_per_partition, int64_t n_rows, int32_t dim, const float *q_loc,
                                const float *q_scale, const float *p_loc, const float *p_scale, float *out_kl, int32_t *out_num,
                                void *workspace, size_t workspace_bytes, void *hip_stream) try {
  using namespace irec;
  const char *who = "irec_fit_partitions";
  if (!ctx) return set_last_error(IREC_E_INVALID, who, "null context");
  irec_fit_params P{kl_per_partition, 0.0, 0.0, 1};
  if (const char *why = fit_check(&P, n_rows, dim)) return set_last_error(IREC_E_INVALID, who, why);
  if (!q_loc || !q_scale || !p_loc || !p_scale || !out_kl || !out_num || !workspace)
    return set_last_error(IREC_E_INVALID, who, "null pointer argument");
  const FitLayout L = fit_layout(n_rows, dim);
  if (workspace_bytes < L.bytes) return set_last_error(IREC_E_WORKSPACE, who, "workspace smaller than irec_fit_workspace_bytes()");
  int prev = -1;
  IREC_HIP(hipGetDevice(&prev));
  const int dev = context_device(ctx);
  if (prev != dev) IREC_HIP(hipSetDevice(dev));
  struct Back { int prev, dev; ~Back() { if (prev != dev) (void)hipSetDevice(prev); } } back{prev, dev};
  hipStream_t st = (hipStream_t)hip_stream;
  char *ws = (char *)workspace;
  FitRowsArgs A{};
  A.mq = q_loc; A.sq = q_scale; A.mp = p_loc; A.sp = p_scale; A.sel = nullptr; A.n_sel = (int32_t)n_rows; A.D = dim;
  A.tot = (double *)(ws + L.tot); A.kl = (float *)(ws + L.kl); A.num = (int32_t *)(ws + L.num); A.omega = kl_per_partition;
  IREC_HIP(launch_fit_rows(A, (int)std::min<int64_t>(n_rows, 8LL * std::max(1, context_cus(ctx))), st));
  IREC_HIP(hipMemcpyAsync(out_kl, A.kl, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
  IREC_HIP(hipMemcpyAsync(out_num, A.num, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
  IREC_HIP(hipStreamSynchronize(st));
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_fit_partitions", e.what()); }

irec_status irec_fit_aux_ratios(irec_context *ctx, const irec_fit_params *p, int64_t n_rows, int32_t dim, const float *q_loc,
                                const float *q_scale, const float *p_loc, const float *p_scale, const float *normal_table,
                                int32_t table_steps, float *ratios, float *average_counts, int32_t capacity, int32_t *length,
                                int32_t *out_iters, void *workspace, size_t workspace_bytes, void *hip_stream) try {
  using namespace irec;
  const char *who = "irec_fit_aux_ratios";
  if (!ctx) return set_last_error(IREC_E_INVALID, who, "null context");
  if (const char *why = fit_check(p, n_rows, dim)) return set_last_error(IREC_E_INVALID, who, why);
  if (!q_loc || !q_scale || !p_loc || !p_scale || !ratios || !average_counts || !length || !workspace)
    return set_last_error(IREC_E_INVALID, who, "null pointer argument");
  if (*length < 1 || *length > capacity) return set_last_error(IREC_E_INVALID, who, "length outside [1, capacity]");
  const FitLayout L = fit_layout(n_rows, dim);
  if (workspace_bytes < L.bytes) return set_last_error(IREC_E_WORKSPACE, who, "workspace smaller than irec_fit_workspace_bytes()");
  const int64_t n = n_rows, D = dim;
  const size_t E = (size_t)n * (size_t)D;
  std::vector<float> kl((size_t)n);
  std::vector<int32_t> num((size_t)n), sel((size_t)n);
  if (irec_status s = irec_fit_partitions(ctx, p->kl_per_partition, n_rows, dim, q_loc, q_scale, p_loc, p_scale, kl.data(), num.data(),
                                          workspace, workspace_bytes, hip_stream)) return s;
  int32_t M = 0;
  if (const char *why = fit_counts(kl.data(), num.data(), n, &M)) return set_last_error(IREC_E_INVALID, who, why);
  const int32_t cur = *length;
  if (std::max(M, cur) > capacity) return set_last_error(IREC_E_INVALID, who, "capacity smaller than the partitions the rows need");
  if (M > 1 && (!normal_table || table_steps < M - 1 || !out_iters)) return set_last_error(IREC_E_INVALID, who, "the normal table covers fewer than M - 1 steps");
  int prev = -1;
  IREC_HIP(hipGetDevice(&prev));
  const int dev = context_device(ctx);
  if (prev != dev) IREC_HIP(hipSetDevice(dev));
  struct Back { int prev, dev; ~Back() { if (prev != dev) (void)hipSetDevice(prev); } } back{prev, dev};
  hipStream_t st = (hipStream_t)hip_stream;
  const int n_cu = std::max(1, context_cus(ctx));
  char *ws = (char *)workspace;
  float *mq = (float *)(ws + L.stats[0]), *sq = (float *)(ws + L.stats[1]), *mp = (float *)(ws + L.stats[2]), *sp = (float *)(ws + L.stats[3]);
  if (M > 1) {
    IREC_HIP(hipMemcpyAsync(mq, q_loc, E * 4, hipMemcpyDeviceToDevice, st));
    IREC_HIP(hipMemcpyAsync(sq, q_scale, E * 4, hipMemcpyDeviceToDevice, st));
    IREC_HIP(hipMemcpyAsync(mp, p_loc, E * 4, hipMemcpyDeviceToDevice, st));
    IREC_HIP(hipMemcpyAsync(sp, p_scale, E * 4, hipMemcpyDeviceToDevice, st));
  }
  for (int32_t i = cur; i < M; ++i) { ratios[i] = 0.0f; average_counts[i] = 0.0f; }
  *length = std::max(M, cur);
  const size_t S_pad = ((size_t)n + IREC_NORMAL_TABLE_PAD - 1) / IREC_NORMAL_TABLE_PAD * IREC_NORMAL_TABLE_PAD;
  const double om = (double)p->kl_per_partition;
  const int chunk = std::max(1, g_fit_chunk.load());
  FitState *d_state = (FitState *)(ws + L.state);
  for (int32_t ratio = M; ratio >= 2; --ratio) {
    const int32_t j = M - ratio;
    int32_t ns = 0;
    for (int64_t i = 0; i < n; ++i) if (num[i] >= ratio) sel[ns++] = (int32_t)i;
    // (pageable source: the copy has left `sel` when the call returns; the stream is drained before `sel` changes anyway)
    IREC_HIP(hipMemcpyAsync(ws + L.sel, sel.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st));
    FitRowsArgs R{};
    R.mq = mq; R.sq = sq; R.mp = mp; R.sp = sp; R.sel = (const int32_t *)(ws + L.sel); R.n_sel = ns; R.D = dim;
    R.tot = (double *)(ws + L.tot); R.W = (double *)(ws + L.W); R.S = (double *)(ws + L.S);
    R.state = d_state; R.theta0 = fit_theta0(ratios, ratio, M);
    IREC_HIP(launch_fit_rows(R, std::min(ns, 8 * n_cu), st));
    FitIterArgs I{};
    I.state = d_state; I.W = R.W; I.S = R.S; I.tot = R.tot; I.pair = (double *)(ws + L.pair);
    I.n_sel = ns; I.D = dim; I.max_iters = p->max_iters; I.om = om; I.om_rest = om * (double)(ratio - 1);
    I.lr = p->learning_rate; I.tol = p->relative_tolerance;
    const int grid = std::min(ns, 4 * n_cu);
    FitState hs{};
    for (int64_t launched = 0; launched < p->max_iters && !hs.done;) {
      const int c = (int)std::min<int64_t>(chunk, p->max_iters - launched);
      for (int i = 0; i < c; ++i) hipLaunchKernelGGL(fit_iter_kernel, dim3(grid), dim3(FIT_NT), 0, st, I);
      IREC_HIP(hipGetLastError());
      launched += c;
      IREC_HIP(hipMemcpyAsync(&hs, d_state, sizeof(hs), hipMemcpyDeviceToHost, st));
      IREC_HIP(hipStreamSynchronize(st));
    }
    if (!hs.done) return set_last_error(IREC_E_HIP, who, "a fit step did not finish within max_iters launches");
    out_iters[j] = hs.iters;
    const float r_last = (float)hs.rho_last;
    const float r_avg = fit_average(ratios, average_counts, ratio, r_last, ns);
    FitHandArgs H{};
    H.mq = mq; H.sq = sq; H.mp = mp; H.sp = sp; H.sel = R.sel; H.tab = normal_table + (size_t)j * (size_t)D * S_pad;
    H.n_sel = ns; H.D = dim; H.S_pad = (int32_t)S_pad; H.r_last = r_last; H.r_avg = r_avg;
    const int64_t hg = ((int64_t)ns * D + FIT_NT - 1) / FIT_NT;
    hipLaunchKernelGGL(fit_handover_kernel, dim3((unsigned)std::min<int64_t>(hg, 16LL * n_cu)), dim3(FIT_NT), 0, st, H);
    IREC_HIP(hipGetLastError());
  }
  IREC_HIP(hipStreamSynchronize(st));   // (the next call may reuse the workspace, and `sel` goes out of scope)
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_fit_aux_ratios", e.what()); }

} // extern "C"
