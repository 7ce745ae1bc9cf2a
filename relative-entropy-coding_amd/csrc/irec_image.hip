// irec_image.hip -- the bilinear shrink of a batch of images on the device and on the host (include/irec.h: irec_resize_bilinear_*):
// tf.image.resize(image, [h - h % 64, w - w % 64]) of the reference's lossy driver (examples/lossy/compress_with_lossy_model.py:183-184).
// The arithmetic and the walk of a tile are csrc/irec_image_core.h; the kernel here is one lane of it per thread, and the host entry at
// the end of this file runs the same lanes over host memory.
//
// One launch, one 64-thread workgroup per tile of 16 rows x 64 consecutive row elements of one plane's output: a lane computes its
// column's taps and weight once, walks the tile's rows and keeps the lower source row's value for the next row, so a shrink by less
// than 2 loads two taps per output.  Lanes of a wave read neighbouring elements of the same source rows (coalesced up to the shrink
// factor; the second tap of a lane is the first of its neighbour, from the same cache lines) and write consecutive elements.  The source
// rows are NOT staged in LDS: a tile's span of the source is unbounded in the shrink factor, and a source line is used by the lanes of
// one wave at one time, which the vector cache serves; the staged form exists as a diagnostic build (IREC_IMAGE_STAGE below, the
// core header's phase_stage) and is measured beside this one in profiles/resize/bench.json.  No atomics, no
// workspace: every store goes to an element that only its lane owns, and an image's result does not depend on what is beside it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>

#include "irec_call.h"
#include "irec_image_core.h"

namespace irec {
namespace {
namespace I = irec_image;

#ifndef IREC_IMAGE_STAGE
#define IREC_IMAGE_STAGE 0      // 1: the diagnostic build that stages a tile's source rectangle in LDS (make variant_image; scripts/bench_resize.py --variant)
#endif

#if IREC_IMAGE_STAGE
__global__ __launch_bounds__(I::NT) void resize_bilinear_kernel(I::Call k) {
  __shared__ I::Stage m;
  const I::Tile T = I::tile_of(k, blockIdx.x);
  const I::Span s = I::span_of(k, T);                     // (the same for every lane of the workgroup)
  if (!s.fits) { I::lane_of_tile(k, blockIdx.x, threadIdx.x); return; }
  I::phase_stage(k, T, s, m, threadIdx.x);
  __syncthreads();
  I::lane_walk(k, T, threadIdx.x, I::Staged{m, s});
}
#else
__global__ __launch_bounds__(I::NT) void resize_bilinear_kernel(I::Call k) { I::lane_of_tile(k, blockIdx.x, threadIdx.x); }
#endif

// IREC_OK, or the argument error of both entries
irec_status check_args(const char *who, const void *src, int32_t src_dtype, int32_t n, int32_t c, int32_t in_h, int32_t in_w, int32_t out_h,
                       int32_t out_w, int32_t layout, const float *dst) {
  if (!src || !dst) return set_last_error(IREC_E_INVALID, who, "null pointer");
  if (const char *what = I::shape_error(n, c, in_h, in_w, out_h, out_w, layout, src_dtype)) return set_last_error(IREC_E_INVALID, who, what);
  if (((uintptr_t)dst & 3) || (src_dtype == IREC_IMAGE_F32 && ((uintptr_t)src & 3))) return set_last_error(IREC_E_INVALID, who, "a float32 array that is not 4-byte aligned");
  return IREC_OK;
}
} // namespace
} // namespace irec

extern "C" {

irec_status irec_resize_bilinear_device(const void *src, int32_t src_dtype, int32_t n, int32_t c, int32_t in_h, int32_t in_w, int32_t out_h,
                                        int32_t out_w, int32_t layout, float *dst, void *hip_stream) {
  using namespace irec;
  if (irec_status st = check_args("irec_resize_bilinear_device", src, src_dtype, n, c, in_h, in_w, out_h, out_w, layout, dst)) return st;
  I::Call call;
  I::bind(call, src, src_dtype, n, c, in_h, in_w, out_h, out_w, layout, dst);
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)call.tiles()), dim3(I::NT), 0, (hipStream_t)hip_stream, call);
  IREC_HIP(hipGetLastError());
  return IREC_OK;
}

irec_status irec_resize_bilinear_host(const void *src, int32_t src_dtype, int32_t n, int32_t c, int32_t in_h, int32_t in_w, int32_t out_h,
                                      int32_t out_w, int32_t layout, float *dst, int32_t n_threads) try {
  using namespace irec;
  if (irec_status st = check_args("irec_resize_bilinear_host", src, src_dtype, n, c, in_h, in_w, out_h, out_w, layout, dst)) return st;
  I::Call call;
  I::bind(call, src, src_dtype, n, c, in_h, in_w, out_h, out_w, layout, dst);
  I::call_host(call, Chunks{n_threads, 16});   // (a thread is not worth fewer than 16 tiles)
  return IREC_OK;
} catch (const std::exception &e) { return irec::set_last_error(IREC_E_INVALID, "irec_resize_bilinear_host", e.what()); }

} // extern "C"
