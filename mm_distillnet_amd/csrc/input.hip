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

// ---- training-time augmentation in front of Normalizer + Resizer, a whole stacked batch of one modality per launch
//
//   shift      (src/datasets/MultimodalDetection.py:236-242,320-327): img_new[:, 0:W-shift] = img[:, shift:], the rest 0.  Upstream shifts
//              AFTER the thermal stretch and the /255, so a vacated pixel is 0 in the stretched frame (for uint8 frames: a raw 0)
//   HSVAdjust  (src/datasets/transformations.py:133-190): rgb/255 -> cv2.cvtColor(RGB2HSV) -> h += hue, wrapped once into [0, 360) ->
//              s = clip(sat*s, 0, 1), v = clip(val*v, 0, 1) -> cv2.cvtColor(HSV2RGB) -> *255 (no rounding)
//
// cv2.cvtColor is restated from OpenCV's documented float formulas (V = max, S = (V - min)/V or 0 at V = 0, H = 60(G-B)/(V-min) at V = R,
// 120 + 60(B-R)/(V-min) at V = G, 240 + 60(R-G)/(V-min) at V = B - the maximal channel taken in R, G, B order -, + 360 if negative, 0 where
// max = min; the inverse is the six-sector form).  Like the resize rules above, parity with cv2 itself is UNPINNED (its float code adds
// FLT_EPSILON to both divisors); the kernel is held to the project's own restatement, tests/hsv_ref.py.
//
// Row b of aug[B, 5] = (on, hue_deg, sat, val, shift_px).  The adjusted pixels are RECOMPUTED per bilinear tap (4 conversions per output
// pixel), not staged in LDS: see DESIGN.md, kernel notes of f3.
__device__ __forceinline__ void hsv_adjust(float& r, float& g, float& b, float hue, float sat, float val) {
  r = r / 255.f; g = g / 255.f; b = b / 255.f;
  const float v = fmaxf(r, fmaxf(g, b)), d = v - fminf(r, fminf(g, b));
  float s = v != 0.f ? d / v : 0.f, h = 0.f;
  if (d != 0.f) {
    if (v == r) h = 60.f * (g - b) / d;
    else if (v == g) h = 120.f + 60.f * (b - r) / d;
    else h = 240.f + 60.f * (r - g) / d;
    if (h < 0.f) h += 360.f;
  }
  h += hue;
  if (h >= 360.f) h -= 360.f;                // clip_hue: one wrap each way, in this order
  if (h < 0.f) h += 360.f;
  s = fminf(fmaxf(sat * s, 0.f), 1.f);
  const float vv = fminf(fmaxf(val * v, 0.f), 1.f);
  const float hs = h / 60.f, fl = floorf(hs), f = hs - fl;
  int sec = (int)fl % 6;                     // h = 360 after the wrap (a tiny negative hue + 360 in fp32) is sector 0 with f = 0
  if (sec < 0) sec += 6;
  const float p = vv * (1.f - s), q = vv * (1.f - s * f), t = vv * (1.f - s * (1.f - f));
  switch (sec) {
    case 0: r = vv; g = t; b = p; break;
    case 1: r = q; g = vv; b = p; break;
    case 2: r = p; g = vv; b = t; break;
    case 3: r = p; g = q; b = vv; break;
    case 4: r = t; g = p; b = vv; break;
    default: r = vv; g = p; b = q; break;
  }
  r *= 255.f; g *= 255.f; b *= 255.f;
}

// Normalizer's (v * scale - mean) * inv_std and the bilinear blends a * (1 - w) + b * w, with the contraction hipcc gives those expressions
// in image_letterbox_kernel (fma(v, scale, -mean) * inv_std; fma(a, 1 - w, b * w)) SPELLED OUT: left to the optimiser, this kernel's merged
// branch tails came out as mul + sub for one channel, and an un-augmented sample must have mmd_image_letterbox's bits.
__device__ __forceinline__ float aug_norm(float v, int c, const ImgPre& p) { return fmaf(v, p.scale, -p.mean[c]) * p.inv_std[c]; }
__device__ __forceinline__ float aug_lerp(float a, float b, float w) { return fmaf(a, 1.f - w, b * w); }

// one source pixel (sy, sx) of the shifted, adjusted, normalised frame -> out[0..C)
template <int C, bool HSV>
__device__ __forceinline__ void aug_pixel(const void* src, const ImgPre& p, int W, int sy, int sx, int shift, bool on, float hue,
                                          float sat, float val, float mn, float k, float out[C]) {
  constexpr int DT = C == 3 ? 0 : 1;         // the entry point's formats: 3 x uint8 or 1 x uint16 (a constant: img_load's branches fold)
  sx += shift;                               // shift <= W: no overflow
  if (sx >= W) {                             // vacated column: 0 in the stretched frame (and black stays black under HSVAdjust)
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = aug_norm(0.f, c, p);
    return;
  }
  const size_t i = ((size_t)sy * W + sx) * C;
  if constexpr (HSV) {                       // (C == 3, no min-max stretch: the entry point refuses anything else)
    if (on) {
      float r = img_load(src, DT, i), g = img_load(src, DT, i + 1), b = img_load(src, DT, i + 2);
      hsv_adjust(r, g, b, hue, sat, val);
      out[0] = aug_norm(r, 0, p); out[1] = aug_norm(g, 1, p); out[2] = aug_norm(b, 2, p);
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float v = img_load(src, DT, i + c);
    if (C == 1 && p.minmax) v = rintf((fminf(fmaxf(v, p.lo), p.hi) - mn) * k);      // img_pre's stretch (thermal only)
    out[c] = aug_norm(v, c, p);
  }
}

// blockIdx.z = the sample: src[B, H, W, C] -> dst[B, C, S, S]; one thread = all C channels of one output pixel (HSV couples them).
// A sample with on == 0 and shift == 0 runs image_letterbox_kernel's arithmetic (as compiled: aug_norm, aug_lerp) on its operands: the same bits.
template <int C, bool HSV>
__global__ __launch_bounds__(256) void image_letterbox_aug_kernel(const void* __restrict__ src, int H, int W, ImgPre p,
                                                                  const float* __restrict__ aug, int rh, int rw, int S,
                                                                  float* __restrict__ dst) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, bz = blockIdx.z;
  if (x >= S) return;
  constexpr size_t elt = C == 3 ? 1 : 2;     // uint8 x 3 or uint16 x 1
  src = reinterpret_cast<const char*>(src) + (size_t)bz * H * W * C * elt;
  dst += (size_t)bz * C * S * S;
  const float* a = aug + (size_t)bz * 5;
  const bool on = HSV && a[0] != 0.f;
  const float hue = a[1], sat = a[2], val = a[3];
  const int shift = min(max((int)a[4], 0), W);
  float mn = 0.f, k = 1.f;
  if (p.minmax) { mn = p.mm[2 * bz]; float mx = p.mm[2 * bz + 1]; k = mx > mn ? 255.f / (mx - mn) : 0.f; }
  if (y >= rh || x >= rw) {
#pragma unroll
    for (int c = 0; c < C; ++c) dst[((size_t)c * S + y) * S + x] = 0.f;
    return;
  }
  double fy = ((double)y + 0.5) * ((double)H / rh) - 0.5, fx = ((double)x + 0.5) * ((double)W / rw) - 0.5;
  int sy = (int)floor(fy), sx = (int)floor(fx);
  float wy = (float)(fy - sy), wx = (float)(fx - sx);
  if (sy < 0) { sy = 0; wy = 0.f; }
  if (sy >= H - 1) { sy = H - 1; wy = 0.f; }
  if (sx < 0) { sx = 0; wx = 0.f; }
  if (sx >= W - 1) { sx = W - 1; wx = 0.f; }
  const int sy1 = min(sy + 1, H - 1), sx1 = min(sx + 1, W - 1);
  float v00[C], v01[C], v10[C], v11[C];
  aug_pixel<C, HSV>(src, p, W, sy, sx, shift, on, hue, sat, val, mn, k, v00);
  aug_pixel<C, HSV>(src, p, W, sy, sx1, shift, on, hue, sat, val, mn, k, v01);
  aug_pixel<C, HSV>(src, p, W, sy1, sx, shift, on, hue, sat, val, mn, k, v10);
  aug_pixel<C, HSV>(src, p, W, sy1, sx1, shift, on, hue, sat, val, mn, k, v11);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float top = aug_lerp(v00[c], v01[c], wx), bot = aug_lerp(v10[c], v11[c], wx);       // horizontal pass, then vertical
    dst[((size_t)c * S + y) * S + x] = aug_lerp(top, bot, wy);
  }
}

extern "C" int mmd_image_letterbox_aug_batch(const void* src, int B, int H, int W, int C, float scale, const float* mean,
                                             const float* stdv, int minmax, float lo, float hi, const float* mm, const float* aug,
                                             int hsv, int common_size, float* dst, hipStream_t stream) {
  if (!src || !dst || !aug || B < 1 || B > 65535 || H < 1 || W < 1 || common_size < 1 || common_size > 65535) return MMD_EINVAL;
  if (C != 1 && C != 3) return MMD_EINVAL;
  if (hsv && C != 3) return MMD_EINVAL;      // HSVAdjust is a colour transform: the 1-channel thermal frame takes the shift only
  if (minmax && (C != 1 || !mm || hi < lo)) return MMD_EINVAL;
  ImgPre p{};
  p.dtype = C == 3 ? 0 : 1; p.scale = scale; p.minmax = minmax; p.lo = lo; p.hi = hi; p.mm = mm;
  for (int c = 0; c < 4; ++c) { p.mean[c] = (mean && c < C) ? mean[c] : 0.f; p.inv_std[c] = (stdv && c < C) ? 1.f / stdv[c] : 1.f; }
  int rh, rw;                                // Resizer's geometry, as in mmd_image_letterbox
  if (H > W) { double s = (double)common_size / H; rh = common_size; rw = (int)(W * s); }
  else { double s = (double)common_size / W; rh = (int)(H * s); rw = common_size; }
  if (rh < 1 || rw < 1) return MMD_EINVAL;
  const dim3 grid(cdiv(common_size, 256), common_size, B), block(256);
  if (C == 1) hipLaunchKernelGGL((image_letterbox_aug_kernel<1, false>), grid, block, 0, stream, src, H, W, p, aug, rh, rw, common_size, dst);
  else if (hsv) hipLaunchKernelGGL((image_letterbox_aug_kernel<3, true>), grid, block, 0, stream, src, H, W, p, aug, rh, rw, common_size, dst);
  else hipLaunchKernelGGL((image_letterbox_aug_kernel<3, false>), grid, block, 0, stream, src, H, W, p, aug, rh, rw, common_size, dst);
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
