// irec_res.hip -- the .res container on the device and on the host: a batch's pixels coded under the model's likelihood given the
// reconstructions, and read back into exactly those pixels (include/irec.h: irec_res_*).  The model and the coder are
// csrc/irec_res_core.h; the kernels here only deal its lane functions out, and the host entry points at the end of this file run the
// same functions over host memory, so that a file is the same bytes wherever it was made.
//
// One lane per stream, N n_streams streams per call, lane i n_streams + j.  256-lane workgroups, plain launches, no atomics: every
// store goes into a byte range that only its lane owns.
//   encode:  res_size_kernel (input checks, bits and checksum share of every stream) -> res_layout_kernel (bytes per file, exclusive
//            scan: offsets, status, stream positions, headers) -> res_write_kernel (streams; nothing at all if the files do not fit cap)
//   decode:  res_decode_head_kernel (header checks, stream positions) -> res_decode_streams_kernel (pixels, checksum shares)
//            -> res_decode_status_kernel (one status per image, first cause; the pixels of an image with an error zeroed)
// The "_scales" entry points (one scale per channel, version-2 files) run the same launches through kernels of their own, compiled with
// irec_res::ChannelScales where those above are compiled with irec_res::CallScale.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <thread>
#include <vector>

#include "irec_res_core.h"

namespace irec {
irec_status set_last_error(irec_status code, const char *who, const char *what);   // irec_host.cpp

namespace {
constexpr int RES_NT = 256;

__global__ __launch_bounds__(RES_NT) void res_size_kernel(irec_res::EncodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::encode_size_lane(c, lane);
}

// One workgroup: lane t takes the images [t * per, (t + 1) * per), so any N is covered; the 256 partial sums are scanned in LDS.
__global__ __launch_bounds__(RES_NT) void res_layout_kernel(irec_res::EncodeCall c) {
  __shared__ int64_t part[RES_NT];
  const int t = threadIdx.x;
  const int64_t per = ((int64_t)c.N + RES_NT - 1) / RES_NT, lo = t * per, hi = lo + per < c.N ? lo + per : c.N;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += irec_res::encode_image_bytes(c, i);   // (also leaves status[i])
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < RES_NT; d *= 2) {
    const int64_t add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  const int64_t total = part[RES_NT - 1];
  int64_t at = part[t] - sum;                                                    // exclusive
  // the sizes once more, from the statuses just written by this very lane
  for (int64_t i = lo; i < hi; ++i) { irec_res::encode_image_layout(c, i, at, total <= c.cap); at += irec_res::encode_image_bytes(c, i); }
  if (t == RES_NT - 1) c.offsets[c.N] = total;
}

__global__ __launch_bounds__(RES_NT) void res_write_kernel(irec_res::EncodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::encode_write_lane(c, lane);
}

__global__ __launch_bounds__(RES_NT) void res_decode_head_kernel(irec_res::DecodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < c.N) irec_res::decode_head_lane(c, lane);
}

__global__ __launch_bounds__(RES_NT) void res_decode_streams_kernel(irec_res::DecodeCall c) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::decode_stream_lane(c, lane);
}

// One workgroup per image: the header's cause, else the first failing stream's, else the checksum's; zeroed pixels if there is one.
__global__ __launch_bounds__(RES_NT) void res_decode_status_kernel(irec_res::DecodeCall c) {
  __shared__ int64_t first[RES_NT];
  __shared__ uint32_t sums[RES_NT];
  const int t = threadIdx.x;
  constexpr int64_t NONE = 0x7fffffffffffffffll;
  for (int64_t i = blockIdx.x; i < c.N; i += gridDim.x) {
    int64_t mine = NONE;                                                         // (j << 8 | status) of the first failing stream this lane saw
    uint32_t sum = 0;
    for (int64_t j = t; j < c.ns; j += RES_NT) {
      const int32_t st = c.stream_status[i * c.ns + j];
      if (st && mine == NONE) mine = (j << 8) | st;
      sum += c.share[i * c.ns + j];
    }
    first[t] = mine; sums[t] = sum;
    __syncthreads();
    for (int d = RES_NT / 2; d > 0; d /= 2) {
      if (t < d) { if (first[t + d] < first[t]) first[t] = first[t + d]; sums[t] += sums[t + d]; }
      __syncthreads();
    }
    int32_t st = c.head_status[i];
    if (!st && first[0] != NONE) st = (int32_t)(first[0] & 0xff);
    if (!st && sums[0] != c.head_sum[i]) st = IREC_RES_E_CHECKSUM;
    __syncthreads();
    if (t == 0) c.status[i] = st;
    if (st) for (int64_t e = t; e < c.n_sym; e += RES_NT) c.pixels[i * c.n_sym + e] = 0;
  }
}

// ---- the same launches under one scale per channel (version 2; irec_res::ChannelScales, scales [channels] on the device): kernels of
//      their own, so that the ones above stay the code they were ----------------------------------------------------------------------
__global__ __launch_bounds__(RES_NT) void res_size_scales_kernel(irec_res::EncodeCall c, irec_res::ChannelScales sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::encode_size_lane(c, sc, lane);
}

__global__ __launch_bounds__(RES_NT) void res_layout_scales_kernel(irec_res::EncodeCall c, irec_res::ChannelScales sc) {
  __shared__ int64_t part[RES_NT];
  const int t = threadIdx.x;
  const int64_t per = ((int64_t)c.N + RES_NT - 1) / RES_NT, lo = t * per, hi = lo + per < c.N ? lo + per : c.N;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += irec_res::encode_image_bytes(c, sc, i);
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < RES_NT; d *= 2) {
    const int64_t add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  const int64_t total = part[RES_NT - 1];
  int64_t at = part[t] - sum;
  for (int64_t i = lo; i < hi; ++i) { irec_res::encode_image_layout(c, sc, i, at, total <= c.cap); at += irec_res::encode_image_bytes(c, sc, i); }
  if (t == RES_NT - 1) c.offsets[c.N] = total;
}

__global__ __launch_bounds__(RES_NT) void res_write_scales_kernel(irec_res::EncodeCall c, irec_res::ChannelScales sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::encode_write_lane(c, sc, lane);
}

__global__ __launch_bounds__(RES_NT) void res_decode_head_scales_kernel(irec_res::DecodeCall c, irec_res::ChannelScales sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < c.N) irec_res::decode_head_lane(c, sc, lane);
}

__global__ __launch_bounds__(RES_NT) void res_decode_streams_scales_kernel(irec_res::DecodeCall c, irec_res::ChannelScales sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::decode_stream_lane(c, sc, lane);
}

int res_grid(int64_t lanes) { const int64_t g = (lanes + RES_NT - 1) / RES_NT; return (int)(g < 1 ? 1 : g); }

// the shape of a call: symbols per image and streams per image, or false
bool shape_ok(int32_t N, uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, int64_t *n_sym, int64_t *ns) {
  if (N < 0 || height < 1 || width < 1 || channels < 1 || height > 65535 || width > 65535 || channels > 65535 || stream_len < 1 ||
      stream_len > irec_res::MAX_STREAM_LEN)
    return false;
  *n_sym = (int64_t)height * width * channels;
  if (*n_sym >= ((int64_t)1 << 31)) return false;
  *ns = irec_res::n_streams_of(*n_sym, stream_len);
  return *ns < ((int64_t)1 << 31) && ((int64_t)N * *ns) / RES_NT < 0x7fffffff;
}

bool make_encode_call(irec_res::EncodeCall &c, const uint8_t *pixels, const float *loc, float scale, int32_t N, uint32_t height, uint32_t width,
                      uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status) {
  int64_t n_sym = 0, ns = 0;
  if (!shape_ok(N, height, width, channels, stream_len, &n_sym, &ns) || !offsets || cap < 0 || (cap > 0 && !out) ||
      (N > 0 && (!pixels || !loc || !status)))
    return false;
  c = irec_res::EncodeCall{pixels, loc, scale, N, (int32_t)ns, height, width, channels, stream_len, n_sym, out, cap, offsets, status,
                           nullptr, nullptr, nullptr, nullptr};
  return true;
}
bool make_decode_call(irec_res::DecodeCall &c, const uint8_t *bytes, const int64_t *offsets, const float *loc, float scale, int32_t N,
                      uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels, int32_t *status) {
  int64_t n_sym = 0, ns = 0;
  if (!shape_ok(N, height, width, channels, stream_len, &n_sym, &ns) || !bytes || !offsets || (N > 0 && (!loc || !pixels || !status)))
    return false;
  c = irec_res::DecodeCall{bytes, offsets, loc, scale, N, (int32_t)ns, height, width, channels, stream_len, n_sym, pixels, status,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  return true;
}

// the lanes of a launch on T host threads, for irec_res_core.h's call forms (body must not throw)
struct ThreadedLanes {
  int32_t n_threads;
  template <class F>
  void operator()(int64_t n, F &&body) const {
    int64_t T = n_threads > 0 ? n_threads : (int64_t)std::thread::hardware_concurrency();
    T = T < 1 ? 1 : (T > 32 ? 32 : T);
    if (T > n / 64) T = n / 64;                                                  // (a thread is not worth fewer than 64 lanes)
    if (T <= 1) { body((int64_t)0, n); return; }
    std::vector<std::thread> pool;
    const int64_t per = (n + T - 1) / T;
    for (int64_t t = 0; t < T; ++t)
      pool.emplace_back([&body, t, per, n]() { const int64_t lo = t * per, hi = lo + per < n ? lo + per : n; if (lo < hi) body(lo, hi); });
    for (auto &th : pool) th.join();
  }
};
} // namespace
} // namespace irec

#define RES_HIP(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return irec::set_last_error(IREC_E_HIP, #expr, hipGetErrorString(e_));         \
  } while (0)

extern "C" {

size_t irec_res_device_workspace_bytes(int32_t n_images, int64_t n_streams) {
  if (n_images < 0 || n_streams < 1) return 0;
  return (size_t)(irec_res::workspace_bytes(n_images, n_streams) + 256);
}

irec_status irec_res_encode_files_device(const uint8_t *pixels, const float *loc, float scale, int32_t n_images, uint32_t height,
                                         uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets,
                                         int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  irec_res::EncodeCall c;
  if (!make_encode_call(c, pixels, loc, scale, n_images, height, width, channels, stream_len, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_res_encode_files_device", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_res_device_workspace_bytes(n_images, c.ns))
    return set_last_error(IREC_E_WORKSPACE, "irec_res_encode_files_device", "workspace too small (irec_res_device_workspace_bytes) or not 8-byte aligned");
  irec_res::encode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t lanes = (int64_t)n_images * c.ns;
  if (lanes > 0) {
    hipLaunchKernelGGL(res_size_kernel, dim3(res_grid(lanes)), dim3(RES_NT), 0, st, c);
    RES_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(res_layout_kernel, dim3(1), dim3(RES_NT), 0, st, c);
  RES_HIP(hipGetLastError());
  if (lanes > 0) {
    hipLaunchKernelGGL(res_write_kernel, dim3(res_grid(lanes)), dim3(RES_NT), 0, st, c);
    RES_HIP(hipGetLastError());
  }
  return IREC_OK;
}

irec_status irec_res_decode_files_device(const uint8_t *bytes, const int64_t *offsets, const float *loc, float scale, int32_t n_images,
                                         uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                         int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  using namespace irec;
  irec_res::DecodeCall c;
  if (!make_decode_call(c, bytes, offsets, loc, scale, n_images, height, width, channels, stream_len, pixels_out, status))
    return set_last_error(IREC_E_INVALID, "irec_res_decode_files_device", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_res_device_workspace_bytes(n_images, c.ns))
    return set_last_error(IREC_E_WORKSPACE, "irec_res_decode_files_device", "workspace too small (irec_res_device_workspace_bytes) or not 8-byte aligned");
  if (n_images == 0) return IREC_OK;
  irec_res::decode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(res_decode_head_kernel, dim3(res_grid(n_images)), dim3(RES_NT), 0, st, c);
  RES_HIP(hipGetLastError());
  hipLaunchKernelGGL(res_decode_streams_kernel, dim3(res_grid((int64_t)n_images * c.ns)), dim3(RES_NT), 0, st, c);
  RES_HIP(hipGetLastError());
  hipLaunchKernelGGL(res_decode_status_kernel, dim3(n_images < 65536 ? n_images : 65536), dim3(RES_NT), 0, st, c);
  RES_HIP(hipGetLastError());
  return IREC_OK;
}

// ---- one scale per channel: version-2 files (scales [channels]: a device pointer here, a host pointer in the host forms below) -------
irec_status irec_res_encode_files_device_scales(const uint8_t *pixels, const float *loc, const float *scales, int32_t n_images,
                                                uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out,
                                                int64_t cap, int64_t *offsets, int32_t *status, void *workspace, size_t workspace_bytes,
                                                void *hip_stream) {
  using namespace irec;
  irec_res::EncodeCall c;
  if (!scales || !make_encode_call(c, pixels, loc, 0.0f, n_images, height, width, channels, stream_len, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_res_encode_files_device_scales", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_res_device_workspace_bytes(n_images, c.ns))
    return set_last_error(IREC_E_WORKSPACE, "irec_res_encode_files_device_scales", "workspace too small (irec_res_device_workspace_bytes) or not 8-byte aligned");
  irec_res::encode_bind_workspace(c, workspace);
  const irec_res::ChannelScales sc{scales, (int64_t)height * width};
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t lanes = (int64_t)n_images * c.ns;
  if (lanes > 0) {
    hipLaunchKernelGGL(res_size_scales_kernel, dim3(res_grid(lanes)), dim3(RES_NT), 0, st, c, sc);
    RES_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(res_layout_scales_kernel, dim3(1), dim3(RES_NT), 0, st, c, sc);
  RES_HIP(hipGetLastError());
  if (lanes > 0) {
    hipLaunchKernelGGL(res_write_scales_kernel, dim3(res_grid(lanes)), dim3(RES_NT), 0, st, c, sc);
    RES_HIP(hipGetLastError());
  }
  return IREC_OK;
}

irec_status irec_res_decode_files_device_scales(const uint8_t *bytes, const int64_t *offsets, const float *loc, const float *scales,
                                                int32_t n_images, uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len,
                                                uint8_t *pixels_out, int32_t *status, void *workspace, size_t workspace_bytes,
                                                void *hip_stream) {
  using namespace irec;
  irec_res::DecodeCall c;
  if (!scales || !make_decode_call(c, bytes, offsets, loc, 0.0f, n_images, height, width, channels, stream_len, pixels_out, status))
    return set_last_error(IREC_E_INVALID, "irec_res_decode_files_device_scales", "bad arguments");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < irec_res_device_workspace_bytes(n_images, c.ns))
    return set_last_error(IREC_E_WORKSPACE, "irec_res_decode_files_device_scales", "workspace too small (irec_res_device_workspace_bytes) or not 8-byte aligned");
  if (n_images == 0) return IREC_OK;
  irec_res::decode_bind_workspace(c, workspace);
  const irec_res::ChannelScales sc{scales, (int64_t)height * width};
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(res_decode_head_scales_kernel, dim3(res_grid(n_images)), dim3(RES_NT), 0, st, c, sc);
  RES_HIP(hipGetLastError());
  hipLaunchKernelGGL(res_decode_streams_scales_kernel, dim3(res_grid((int64_t)n_images * c.ns)), dim3(RES_NT), 0, st, c, sc);
  RES_HIP(hipGetLastError());
  hipLaunchKernelGGL(res_decode_status_kernel, dim3(n_images < 65536 ? n_images : 65536), dim3(RES_NT), 0, st, c);   // (no scale in it)
  RES_HIP(hipGetLastError());
  return IREC_OK;
}

irec_status irec_res_encode_files_scales(const uint8_t *pixels, const float *loc, const float *scales, int32_t n_images, uint32_t height,
                                         uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets,
                                         int32_t *status, int32_t n_threads) try {
  using namespace irec;
  irec_res::EncodeCall c;
  if (!scales || !make_encode_call(c, pixels, loc, 0.0f, n_images, height, width, channels, stream_len, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_res_encode_files_scales", "bad arguments");
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(n_images, c.ns) / 8 + 1));
  irec_res::encode_bind_workspace(c, ws.data());
  irec_res::encode_call_host(c, irec_res::ChannelScales{scales, (int64_t)height * width}, ThreadedLanes{n_threads});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_res_encode_files_scales", e.what()); }

irec_status irec_res_decode_files_scales(const uint8_t *bytes, const int64_t *offsets, const float *loc, const float *scales, int32_t n_images,
                                         uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                         int32_t *status, int32_t n_threads) try {
  using namespace irec;
  irec_res::DecodeCall c;
  if (!scales || !make_decode_call(c, bytes, offsets, loc, 0.0f, n_images, height, width, channels, stream_len, pixels_out, status))
    return set_last_error(IREC_E_INVALID, "irec_res_decode_files_scales", "bad arguments");
  if (n_images == 0) return IREC_OK;
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(n_images, c.ns) / 8 + 1));
  irec_res::decode_bind_workspace(c, ws.data());
  irec_res::decode_call_host(c, irec_res::ChannelScales{scales, (int64_t)height * width}, ThreadedLanes{n_threads});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_res_decode_files_scales", e.what()); }

// ---- the same lane functions over host memory: the referee of the kernels above, and the path of host arrays ------------------------------
irec_status irec_res_encode_files(const uint8_t *pixels, const float *loc, float scale, int32_t n_images, uint32_t height, uint32_t width,
                                  uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status,
                                  int32_t n_threads) try {
  using namespace irec;
  irec_res::EncodeCall c;
  if (!make_encode_call(c, pixels, loc, scale, n_images, height, width, channels, stream_len, out, cap, offsets, status))
    return set_last_error(IREC_E_INVALID, "irec_res_encode_files", "bad arguments");
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(n_images, c.ns) / 8 + 1));
  irec_res::encode_bind_workspace(c, ws.data());
  irec_res::encode_call_host(c, ThreadedLanes{n_threads});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_res_encode_files", e.what()); }

irec_status irec_res_decode_files(const uint8_t *bytes, const int64_t *offsets, const float *loc, float scale, int32_t n_images,
                                  uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                  int32_t *status, int32_t n_threads) try {
  using namespace irec;
  irec_res::DecodeCall c;
  if (!make_decode_call(c, bytes, offsets, loc, scale, n_images, height, width, channels, stream_len, pixels_out, status))
    return set_last_error(IREC_E_INVALID, "irec_res_decode_files", "bad arguments");
  if (n_images == 0) return IREC_OK;
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(n_images, c.ns) / 8 + 1));
  irec_res::decode_bind_workspace(c, ws.data());
  irec_res::decode_call_host(c, ThreadedLanes{n_threads});
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_res_decode_files", e.what()); }

irec_status irec_res_model_counts(int32_t m, float scale, uint32_t *cumulative) {
  if (!cumulative || m < -2048 || m > 2047 || !irec_res::scale_ok(scale))
    return irec::set_last_error(IREC_E_INVALID, "irec_res_model_counts", "bad arguments (m in [-2048, 2047], scale in [2^-24, 2^24])");
  const double inv = irec_res::model_inv(scale);
  for (int32_t k = 0; k <= 256; ++k) cumulative[k] = irec_res::cum(m, inv, k);
  return IREC_OK;
}

irec_status irec_res_symbol_counts(const uint8_t *pixels, const float *loc, float scale, int64_t n, uint32_t *count) {
  if (n < 0 || (n > 0 && (!pixels || !loc || !count)) || !irec_res::scale_ok(scale))
    return irec::set_last_error(IREC_E_INVALID, "irec_res_symbol_counts", "bad arguments (scale in [2^-24, 2^24])");
  const double inv = irec_res::model_inv(scale);
  for (int64_t e = 0; e < n; ++e) {
    const int32_t m = irec_res::loc_to_m(loc[e]), x = pixels[e];
    count[e] = irec_res::is_finite(loc[e]) ? irec_res::cum(m, inv, x + 1) - irec_res::cum(m, inv, x) : 0u;
  }
  return IREC_OK;
}

} // extern "C"
