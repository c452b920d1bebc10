// Device-side input preparation: the reference's per-sample CPU transforms restated as two gather kernels, so raw
// decoded frames cross PCIe once (uint8 / uint16) and everything else happens in HBM.
//
//   Normalizer  (src/datasets/transformations.py:315-330):  rgb = (rgb/255 - mean) / std   (ImageNet statistics)
//   thermal     (src/datasets/MultimodalDetection.py:196-211): clamp to [ir_min, ir_max], cv2.normalize(NORM_MINMAX, 0..255)
//               in the source integer type (round-half-even), /255
//   Resizer     (src/datasets/transformations.py:407-467): aspect-preserving cv2.resize(INTER_LINEAR) to
//               (resized_h, resized_w), pasted top-left into a zero common_size x common_size canvas;
//               audio: cv2.resize(INTER_CUBIC) to common_size x common_size
//   __getitem__ (:245-255): HWC -> CHW float32
//
// cv2 is a third-party dependency that is not part of the reference tree nor of this image: the sampling rules below
// restate OpenCV's published resize (pixel centres: src = (dst + 0.5) * src_size/dst_size - 0.5, border taps clamped;
// bicubic kernel A = -0.75).  Parity with cv2 itself is therefore UNPINNED; the kernels are pinned to oracle/input_ref.py.
#include "common.h"

struct ImgPre {
  int dtype;                 // 0 = uint8, 1 = uint16, 2 = float32
  float scale;               // applied first (1/255)
  float mean[4], inv_std[4]; // then (v - mean[c]) * inv_std[c]
  int minmax;                // thermal: clamp + min-max stretch to 0..255 with integer rounding before `scale`
  float lo, hi;
  const float* mm;           // [2] = (min, max) after clamping, produced by mmd_image_minmax
};

__device__ __forceinline__ float img_load(const void* src, int dtype, size_t i) {
  if (dtype == 0) return (float)reinterpret_cast<const unsigned char*>(src)[i];
  if (dtype == 1) return (float)reinterpret_cast<const unsigned short*>(src)[i];
  return reinterpret_cast<const float*>(src)[i];
}
__device__ __forceinline__ float img_pre(float v, int c, const ImgPre& p, float mn, float k) {
  if (p.minmax) {
    v = fminf(fmaxf(v, p.lo), p.hi);
    v = rintf((v - mn) * k);                 // cv2.normalize into the integer source type: saturate_cast = round-half-even
  }
  return (v * p.scale - p.mean[c]) * p.inv_std[c];
}

// dst[c, y, x] (CHW, S x S): bilinear sample of the pre-processed source inside the (rh, rw) window, 0 outside
__global__ __launch_bounds__(256) void image_letterbox_kernel(const void* __restrict__ src, int H, int W, int C, ImgPre p,
                                                              int rh, int rw, int S, float* __restrict__ dst) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= S) return;
  float mn = 0.f, k = 1.f;
  if (p.minmax) { mn = p.mm[0]; float mx = p.mm[1]; k = mx > mn ? 255.f / (mx - mn) : 0.f; }
  if (y >= rh || x >= rw) {
    for (int c = 0; c < C; ++c) dst[((size_t)c * S + y) * S + x] = 0.f;
    return;
  }
  // double for the coordinate like cv2 (scale = src/dst as double), float weights
  double fy = ((double)y + 0.5) * ((double)H / rh) - 0.5, fx = ((double)x + 0.5) * ((double)W / rw) - 0.5;
  int sy = (int)floor(fy), sx = (int)floor(fx);
  float wy = (float)(fy - sy), wx = (float)(fx - sx);
  if (sy < 0) { sy = 0; wy = 0.f; }
  if (sy >= H - 1) { sy = H - 1; wy = 0.f; }
  if (sx < 0) { sx = 0; wx = 0.f; }
  if (sx >= W - 1) { sx = W - 1; wx = 0.f; }
  const int sy1 = min(sy + 1, H - 1), sx1 = min(sx + 1, W - 1);
  for (int c = 0; c < C; ++c) {
    float v00 = img_pre(img_load(src, p.dtype, ((size_t)sy * W + sx) * C + c), c, p, mn, k);
    float v01 = img_pre(img_load(src, p.dtype, ((size_t)sy * W + sx1) * C + c), c, p, mn, k);
    float v10 = img_pre(img_load(src, p.dtype, ((size_t)sy1 * W + sx) * C + c), c, p, mn, k);
    float v11 = img_pre(img_load(src, p.dtype, ((size_t)sy1 * W + sx1) * C + c), c, p, mn, k);
    float top = v00 * (1.f - wx) + v01 * wx, bot = v10 * (1.f - wx) + v11 * wx;       // horizontal pass, then vertical
    dst[((size_t)c * S + y) * S + x] = top * (1.f - wy) + bot * wy;
  }
}

// (min, max) of clamp(src, lo, hi) over one image
__global__ __launch_bounds__(256) void image_minmax_kernel(const void* __restrict__ src, int dtype, size_t n, float lo, float hi,
                                                           float* mm) {
  __shared__ float smn[4], smx[4];
  float mn = INFINITY, mx = -INFINITY;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float v = fminf(fmaxf(img_load(src, dtype, i), lo), hi);
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  mx = wave_max(mx); mn = -wave_max(-mn);
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { mn = fminf(mn, smn[i]); mx = fmaxf(mx, smx[i]); }
    // values are >= 0 (clamped sensor counts): the float bit pattern is monotone as an unsigned integer
    atomicMin(reinterpret_cast<unsigned int*>(mm), __float_as_uint(mn));
    atomicMax(reinterpret_cast<unsigned int*>(mm + 1), __float_as_uint(mx));
  }
}
__global__ void image_minmax_init_u_kernel(float* mm) {
  reinterpret_cast<unsigned int*>(mm)[0] = 0x7f800000u;      // +inf
  reinterpret_cast<unsigned int*>(mm)[1] = 0u;               // 0.0
}
extern "C" int mmd_image_minmax(const void* src, int dtype, long long n, float lo, float hi, float* mm, hipStream_t stream) {
  if (!src || !mm || n <= 0 || dtype < 0 || dtype > 2 || lo < 0.f || hi < lo) return MMD_EINVAL;
  hipLaunchKernelGGL(image_minmax_init_u_kernel, dim3(1), dim3(1), 0, stream, mm);
  int blocks = (int)((n + 256 * 16 - 1) / (256 * 16)); if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(image_minmax_kernel, dim3(blocks), dim3(256), 0, stream, src, dtype, (size_t)n, lo, hi, mm);
  return mmd_check_launch();
}

extern "C" int mmd_image_letterbox(const void* src, int dtype, int H, int W, int C, float scale, const float* mean,
                                   const float* stdv, int minmax, float lo, float hi, const float* mm, int common_size,
                                   float* dst, hipStream_t stream) {
  if (!src || !dst || H <= 0 || W <= 0 || C <= 0 || C > 4 || common_size <= 0 || dtype < 0 || dtype > 2) return MMD_EINVAL;
  if (minmax && (!mm || hi < lo)) return MMD_EINVAL;
  ImgPre p{};
  p.dtype = dtype; p.scale = scale; p.minmax = minmax; p.lo = lo; p.hi = hi; p.mm = mm;
  for (int c = 0; c < 4; ++c) { p.mean[c] = (mean && c < C) ? mean[c] : 0.f; p.inv_std[c] = (stdv && c < C) ? 1.f / stdv[c] : 1.f; }
  // Resizer: the longer side becomes common_size, the other int(side * scale) (truncation, :414-421)
  int rh, rw;
  if (H > W) { double s = (double)common_size / H; rh = common_size; rw = (int)(W * s); }
  else { double s = (double)common_size / W; rh = (int)(H * s); rw = common_size; }
  if (rh < 1 || rw < 1) return MMD_EINVAL;
  hipLaunchKernelGGL(image_letterbox_kernel, dim3(cdiv(common_size, 256), common_size), dim3(256), 0, stream, src, H, W, C, p,
                     rh, rw, common_size, dst);
  return mmd_check_launch();
}

// ---- cv2.resize(INTER_CUBIC): A = -0.75, taps sx-1..sx+2 clamped to the image, separable (horizontal then vertical)
__device__ __forceinline__ void cubic_w(float x, float w[4]) {
  const float A = -0.75f;
  w[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
  w[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  w[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
  w[3] = 1.f - w[0] - w[1] - w[2];
}
// blockIdx.z = the sample of a batch: src[B, h, w, C] -> dst[B, C, S, S]
__global__ __launch_bounds__(256) void resize_cubic_kernel(const float* __restrict__ src, int h, int w, int C, int S,
                                                           float* __restrict__ dst) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= S) return;
  src += (size_t)blockIdx.z * h * w * C;
  dst += (size_t)blockIdx.z * C * S * S;
  double fy = ((double)y + 0.5) * ((double)h / S) - 0.5, fx = ((double)x + 0.5) * ((double)w / S) - 0.5;
  int sy = (int)floor(fy), sx = (int)floor(fx);
  float wy[4], wx[4];
  cubic_w((float)(fy - sy), wy); cubic_w((float)(fx - sx), wx);
  int ys[4], xs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { ys[k] = min(max(sy - 1 + k, 0), h - 1); xs[k] = min(max(sx - 1 + k, 0), w - 1); }
  for (int c = 0; c < C; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* row = src + (size_t)ys[i] * w * C + c;
      float r = row[(size_t)xs[0] * C] * wx[0] + row[(size_t)xs[1] * C] * wx[1] + row[(size_t)xs[2] * C] * wx[2] +
                row[(size_t)xs[3] * C] * wx[3];
      acc += r * wy[i];
    }
    dst[((size_t)c * S + y) * S + x] = acc;
  }
}
extern "C" int mmd_resize_cubic(const float* src, int h, int w, int C, int common_size, float* dst, hipStream_t stream) {
  if (!src || !dst || h <= 0 || w <= 0 || C <= 0 || common_size <= 0) return MMD_EINVAL;
  hipLaunchKernelGGL(resize_cubic_kernel, dim3(cdiv(common_size, 256), common_size), dim3(256), 0, stream, src, h, w, C,
                     common_size, dst);
  return mmd_check_launch();
}
extern "C" int mmd_resize_cubic_batch(const float* src, int batch, int h, int w, int C, int common_size, float* dst, hipStream_t stream) {
  if (!src || !dst || batch <= 0 || batch > 65535 || h <= 0 || w <= 0 || C <= 0 || common_size <= 0 || common_size > 65535)
    return MMD_EINVAL;
  hipLaunchKernelGGL(resize_cubic_kernel, dim3(cdiv(common_size, 256), common_size, batch), dim3(256), 0, stream, src, h, w, C,
                     common_size, dst);
  return mmd_check_launch();
}
