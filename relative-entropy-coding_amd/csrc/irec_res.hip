// irec_res.hip -- the .res container on the device and on the host: a batch's pixels coded under the model's likelihood given the
// reconstructions, and read back into exactly those pixels (include/irec.h: irec_res_*).  The model and the coder are
// csrc/irec_res_core.h; the kernels here only deal its lane functions out, and the host forms run the same functions over host memory,
// so that a file is the same bytes wherever it was made.  Every codec entry point, at the end of this file, is: the call, prepare,
// then the launches here or the host runner.
//
// One lane per stream, N n_streams streams per call, lane i n_streams + j.  256-lane workgroups, plain launches, no atomics: every
// store goes into a byte range that only its lane owns.
//   encode:  res_size_kernel (input checks, bits and checksum share of every stream) -> res_layout_kernel (bytes per file, exclusive
//            scan: offsets, status, stream positions, headers) -> res_write_kernel (streams; nothing at all if the files do not fit cap)
//   decode:  res_decode_head_kernel (header checks, stream positions) -> res_decode_streams_kernel (pixels, checksum shares)
//            -> res_decode_status_kernel (one status per image, first cause; the pixels of an image with an error zeroed)
// A kernel that a scale enters is one body, a template over the scale policy as the core's lane functions are: irec_res::CallScale (the
// call's one scale, version-1 files) or irec_res::ChannelScales (one scale per channel, version-2 files, the "_scales" entry points).
// The two __global__ wrappers of a body exist to keep the symbols and the code of both: profiles, scripts/isa_summary.sh and the
// memory-contract tests know the kernels by name, and scripts/isa_identity.py holds this library's device code to its predecessor's
// (which is why the layout scan stands under both of its names in full).  No scale enters res_decode_status_kernel: it serves both.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <vector>

#include "irec_call.h"
#include "irec_res_core.h"

namespace irec {
namespace {
using irec_res::CallScale;
using irec_res::ChannelScales;
using irec_res::DecodeCall;
using irec_res::EncodeCall;
constexpr int RES_NT = 256;

template <class Scales>
__device__ inline void res_size_body(const EncodeCall &c, const Scales &sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::encode_size_lane(c, sc, lane);
}

template <class Scales>
__device__ inline void res_write_body(const EncodeCall &c, const Scales &sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::encode_write_lane(c, sc, lane);
}

template <class Scales>
__device__ inline void res_decode_head_body(const DecodeCall &c, const Scales &sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < c.N) irec_res::decode_head_lane(c, sc, lane);
}

template <class Scales>
__device__ inline void res_decode_streams_body(const DecodeCall &c, const Scales &sc) {
  const int64_t lane = (int64_t)blockIdx.x * RES_NT + threadIdx.x;
  if (lane < (int64_t)c.N * c.ns) irec_res::decode_stream_lane(c, sc, lane);
}

__global__ __launch_bounds__(RES_NT) void res_size_kernel(EncodeCall c) { res_size_body(c, CallScale{}); }
__global__ __launch_bounds__(RES_NT) void res_write_kernel(EncodeCall c) { res_write_body(c, CallScale{}); }
__global__ __launch_bounds__(RES_NT) void res_decode_head_kernel(DecodeCall c) { res_decode_head_body(c, CallScale{}); }
__global__ __launch_bounds__(RES_NT) void res_decode_streams_kernel(DecodeCall c) { res_decode_streams_body(c, CallScale{}); }
__global__ __launch_bounds__(RES_NT) void res_size_scales_kernel(EncodeCall c, ChannelScales sc) { res_size_body(c, sc); }
__global__ __launch_bounds__(RES_NT) void res_write_scales_kernel(EncodeCall c, ChannelScales sc) { res_write_body(c, sc); }
__global__ __launch_bounds__(RES_NT) void res_decode_head_scales_kernel(DecodeCall c, ChannelScales sc) { res_decode_head_body(c, sc); }
__global__ __launch_bounds__(RES_NT) void res_decode_streams_scales_kernel(DecodeCall c, ChannelScales sc) { res_decode_streams_body(c, sc); }

// One workgroup: lane t takes the images [t * per, (t + 1) * per), so any N is covered; the 256 partial sums are scanned in LDS.
// (Written out twice: as one body under both wrappers the same statements get their registers in another order, and
// scripts/isa_identity.py holds this library's device code to its predecessor's.)
__global__ __launch_bounds__(RES_NT) void res_layout_kernel(EncodeCall c) {
  __shared__ int64_t part[RES_NT];
  const int t = threadIdx.x;
  const int64_t per = ((int64_t)c.N + RES_NT - 1) / RES_NT, lo = t * per, hi = lo + per < c.N ? lo + per : c.N;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += irec_res::encode_image_bytes(c, CallScale{}, i);   // (also leaves status[i])
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
  for (int64_t i = lo; i < hi; ++i) { irec_res::encode_image_layout(c, CallScale{}, i, at, total <= c.cap); at += irec_res::encode_image_bytes(c, CallScale{}, i); }
  if (t == RES_NT - 1) c.offsets[c.N] = total;
}
__global__ __launch_bounds__(RES_NT) void res_layout_scales_kernel(EncodeCall c, ChannelScales sc) {
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

// One workgroup per image: the header's cause, else the first failing stream's, else the checksum's; zeroed pixels if there is one.
// (No scale in it: it serves both.)
__global__ __launch_bounds__(RES_NT) void res_decode_status_kernel(DecodeCall c) {
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

// ---- from an entry point's arguments to a checked call -------------------------------------------------------------------------------
// A call (EncodeCall or DecodeCall) whose other fields hold the entry point's arguments gets its symbols and streams per image, and is
// held to include/irec.h; sc is the entry's scale policy, and an entry that takes an array of scales must be given one.  IREC_OK, or
// IREC_E_INVALID under the entry's name.
inline bool pointers_ok(const EncodeCall &c) { return c.offsets && c.cap >= 0 && (c.cap == 0 || c.out) && (c.N == 0 || (c.pixels && c.loc && c.status)); }
inline bool pointers_ok(const DecodeCall &c) { return c.bytes && c.offsets && (c.N == 0 || (c.loc && c.pixels && c.status)); }
inline bool scales_given(const CallScale &) { return true; }
inline bool scales_given(const ChannelScales &sc) { return sc.scales != nullptr; }

template <class Call>
bool shape_ok(Call &c) {
  if (c.N < 0 || c.height < 1 || c.width < 1 || c.channels < 1 || c.height > 65535 || c.width > 65535 || c.channels > 65535 || c.stream_len < 1 ||
      c.stream_len > irec_res::MAX_STREAM_LEN)
    return false;
  c.n_sym = (int64_t)c.height * c.width * c.channels;
  if (c.n_sym >= ((int64_t)1 << 31)) return false;
  const int64_t ns = irec_res::n_streams_of(c.n_sym, c.stream_len);
  c.ns = (int32_t)ns;
  return ns < ((int64_t)1 << 31) && ((int64_t)c.N * ns) / RES_NT < 0x7fffffff;
}
template <class Call, class Scales>
irec_status prepare(Call &c, const Scales &sc, const char *who) {
  return scales_given(sc) && shape_ok(c) && pointers_ok(c) ? IREC_OK : set_last_error(IREC_E_INVALID, who, "bad arguments");
}
// the same for a device entry: then the workspace
template <class Call, class Scales>
irec_status prepare_device(Call &c, const Scales &sc, const void *workspace, size_t workspace_bytes, const char *who) {
  if (irec_status e = prepare(c, sc, who)) return e;
  return check_workspace(irec_res_device_workspace_bytes(c.N, c.ns), workspace, workspace_bytes, who, "irec_res_device_workspace_bytes");
}

// ---- the three launches of a prepared call; Scales picks the wrapper of each body ------------------------------------------------------
int res_grid(int64_t lanes) { const int64_t g = (lanes + RES_NT - 1) / RES_NT; return (int)(g < 1 ? 1 : g); }

template <class Call, class Scales>
void launch(void (*plain)(Call), void (*scaled)(Call, ChannelScales), int grid, hipStream_t st, const Call &c, const Scales &sc) {
  if constexpr (Scales::per_channel) hipLaunchKernelGGL(scaled, dim3(grid), dim3(RES_NT), 0, st, c, sc);
  else hipLaunchKernelGGL(plain, dim3(grid), dim3(RES_NT), 0, st, c);
}

template <class Scales>
irec_status launch_encode(EncodeCall &c, const Scales &sc, void *workspace, void *hip_stream) {
  irec_res::encode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t lanes = (int64_t)c.N * c.ns;
  if (lanes > 0) {
    launch(res_size_kernel, res_size_scales_kernel, res_grid(lanes), st, c, sc);
    IREC_HIP(hipGetLastError());
  }
  launch(res_layout_kernel, res_layout_scales_kernel, 1, st, c, sc);             // (also of no image: offsets[0])
  IREC_HIP(hipGetLastError());
  if (lanes > 0) {
    launch(res_write_kernel, res_write_scales_kernel, res_grid(lanes), st, c, sc);
    IREC_HIP(hipGetLastError());
  }
  return IREC_OK;
}
template <class Scales>
irec_status launch_decode(DecodeCall &c, const Scales &sc, void *workspace, void *hip_stream) {
  if (c.N == 0) return IREC_OK;
  irec_res::decode_bind_workspace(c, workspace);
  hipStream_t st = (hipStream_t)hip_stream;
  launch(res_decode_head_kernel, res_decode_head_scales_kernel, res_grid(c.N), st, c, sc);
  IREC_HIP(hipGetLastError());
  launch(res_decode_streams_kernel, res_decode_streams_scales_kernel, res_grid((int64_t)c.N * c.ns), st, c, sc);
  IREC_HIP(hipGetLastError());
  hipLaunchKernelGGL(res_decode_status_kernel, dim3(c.N < 65536 ? c.N : 65536), dim3(RES_NT), 0, st, c);
  IREC_HIP(hipGetLastError());
  return IREC_OK;
}

// ---- the same lane functions over host memory, the lanes of a launch dealt to n_threads (a thread is not worth fewer than 64 lanes):
//      the referee of the kernels above, and the path of host arrays --------------------------------------------------------------------
template <class Scales>
irec_status run_encode_host(EncodeCall &c, const Scales &sc, int32_t n_threads, const char *who) try {
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(c.N, c.ns) / 8 + 1));
  irec_res::encode_bind_workspace(c, ws.data());
  irec_res::encode_call_host(c, sc, Chunks{n_threads, 64});
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }

template <class Scales>
irec_status run_decode_host(DecodeCall &c, const Scales &sc, int32_t n_threads, const char *who) try {
  if (c.N == 0) return IREC_OK;
  std::vector<int64_t> ws((size_t)(irec_res::workspace_bytes(c.N, c.ns) / 8 + 1));
  irec_res::decode_bind_workspace(c, ws.data());
  irec_res::decode_call_host(c, sc, Chunks{n_threads, 64});
  return IREC_OK;
} catch (const std::exception &e) { return set_last_error(IREC_E_INVALID, who, e.what()); }
} // namespace
} // namespace irec

using namespace irec;

extern "C" {

size_t irec_res_device_workspace_bytes(int32_t n_images, int64_t n_streams) {
  if (n_images < 0 || n_streams < 1) return 0;
  return (size_t)(irec_res::workspace_bytes(n_images, n_streams) + 256);
}

// ---- the device entries: the call's one scale; one scale per channel (scales [channels], a device pointer) ------------------------------
irec_status irec_res_encode_files_device(const uint8_t *pixels, const float *loc, float scale, int32_t n_images, uint32_t height,
                                         uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets,
                                         int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  EncodeCall c{pixels, loc, scale, n_images, 0, height, width, channels, stream_len, 0, out, cap, offsets, status};
  if (irec_status e = prepare_device(c, CallScale{}, workspace, workspace_bytes, "irec_res_encode_files_device")) return e;
  return launch_encode(c, CallScale{}, workspace, hip_stream);
}

irec_status irec_res_decode_files_device(const uint8_t *bytes, const int64_t *offsets, const float *loc, float scale, int32_t n_images,
                                         uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                         int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream) {
  DecodeCall c{bytes, offsets, loc, scale, n_images, 0, height, width, channels, stream_len, 0, pixels_out, status};
  if (irec_status e = prepare_device(c, CallScale{}, workspace, workspace_bytes, "irec_res_decode_files_device")) return e;
  return launch_decode(c, CallScale{}, workspace, hip_stream);
}

irec_status irec_res_encode_files_device_scales(const uint8_t *pixels, const float *loc, const float *scales, int32_t n_images,
                                                uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out,
                                                int64_t cap, int64_t *offsets, int32_t *status, void *workspace, size_t workspace_bytes,
                                                void *hip_stream) {
  EncodeCall c{pixels, loc, 0.0f, n_images, 0, height, width, channels, stream_len, 0, out, cap, offsets, status};
  const ChannelScales sc{scales, (int64_t)height * width};
  if (irec_status e = prepare_device(c, sc, workspace, workspace_bytes, "irec_res_encode_files_device_scales")) return e;
  return launch_encode(c, sc, workspace, hip_stream);
}

irec_status irec_res_decode_files_device_scales(const uint8_t *bytes, const int64_t *offsets, const float *loc, const float *scales,
                                                int32_t n_images, uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len,
                                                uint8_t *pixels_out, int32_t *status, void *workspace, size_t workspace_bytes,
                                                void *hip_stream) {
  DecodeCall c{bytes, offsets, loc, 0.0f, n_images, 0, height, width, channels, stream_len, 0, pixels_out, status};
  const ChannelScales sc{scales, (int64_t)height * width};
  if (irec_status e = prepare_device(c, sc, workspace, workspace_bytes, "irec_res_decode_files_device_scales")) return e;
  return launch_decode(c, sc, workspace, hip_stream);
}

// ---- the host forms (scales [channels]: a host pointer) ---------------------------------------------------------------------------------
irec_status irec_res_encode_files(const uint8_t *pixels, const float *loc, float scale, int32_t n_images, uint32_t height, uint32_t width,
                                  uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets, int32_t *status,
                                  int32_t n_threads) {
  EncodeCall c{pixels, loc, scale, n_images, 0, height, width, channels, stream_len, 0, out, cap, offsets, status};
  if (irec_status e = prepare(c, CallScale{}, "irec_res_encode_files")) return e;
  return run_encode_host(c, CallScale{}, n_threads, "irec_res_encode_files");
}

irec_status irec_res_decode_files(const uint8_t *bytes, const int64_t *offsets, const float *loc, float scale, int32_t n_images,
                                  uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                  int32_t *status, int32_t n_threads) {
  DecodeCall c{bytes, offsets, loc, scale, n_images, 0, height, width, channels, stream_len, 0, pixels_out, status};
  if (irec_status e = prepare(c, CallScale{}, "irec_res_decode_files")) return e;
  return run_decode_host(c, CallScale{}, n_threads, "irec_res_decode_files");
}

irec_status irec_res_encode_files_scales(const uint8_t *pixels, const float *loc, const float *scales, int32_t n_images, uint32_t height,
                                         uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *out, int64_t cap, int64_t *offsets,
                                         int32_t *status, int32_t n_threads) {
  EncodeCall c{pixels, loc, 0.0f, n_images, 0, height, width, channels, stream_len, 0, out, cap, offsets, status};
  const ChannelScales sc{scales, (int64_t)height * width};
  if (irec_status e = prepare(c, sc, "irec_res_encode_files_scales")) return e;
  return run_encode_host(c, sc, n_threads, "irec_res_encode_files_scales");
}

irec_status irec_res_decode_files_scales(const uint8_t *bytes, const int64_t *offsets, const float *loc, const float *scales, int32_t n_images,
                                         uint32_t height, uint32_t width, uint32_t channels, uint32_t stream_len, uint8_t *pixels_out,
                                         int32_t *status, int32_t n_threads) {
  DecodeCall c{bytes, offsets, loc, 0.0f, n_images, 0, height, width, channels, stream_len, 0, pixels_out, status};
  const ChannelScales sc{scales, (int64_t)height * width};
  if (irec_status e = prepare(c, sc, "irec_res_decode_files_scales")) return e;
  return run_decode_host(c, sc, n_threads, "irec_res_decode_files_scales");
}

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
