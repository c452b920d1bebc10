// Device-side detection record of streaming detection (AudioDetector.detect_stream): the rows decode / NMS leave for one group of
// windows are appended to one caller-owned record behind every group, and the host copies the record once at the end of the recording -
// the shape the evaluation's record has (evalstats.hip), for the rows themselves.
//
// One 256-thread block per call.  ctl = {n_valid, first_window} is read on the device, so one captured graph serves every group of a
// recording: the host only swaps the control block between replays.  The offsets are an exclusive scan of the (clamped) counts of the
// images 0 .. n_valid-1 on top of *rec_count, done by one thread (B is a batch size, at most DR_BMAX), so the order - image, then the
// NMS output order within the image - and with it every bit of the record is the same in every run: no atomics.  *rec_count advances
// by the true total even behind rec_cap; rows that do not fit are not written and *rec_overflow is set (sticky), so the host can name
// the rows needed.  Plain vector stores only.
#include "common.h"

#define DR_BMAX 1024

__global__ __launch_bounds__(256) void det_record_append_kernel(const float* __restrict__ rows, const int* __restrict__ cnt, int B,
                                                                int cap_img, const int* __restrict__ ctl, float* __restrict__ rec_rows,
                                                                int* __restrict__ rec_win, int rec_cap, int* __restrict__ rec_count,
                                                                int* __restrict__ rec_overflow) {
  __shared__ long long s_off[DR_BMAX + 1];      // s_off[i]: record row of image i's first row; s_off[n_valid]: the new count
  __shared__ int s_nv;
  const int tid = threadIdx.x;
  if (tid == 0) {
    const int nv = max(0, min(ctl[0], B));
    long long o = max(*rec_count, 0);
    for (int i = 0; i < nv; ++i) {
      s_off[i] = o;
      o += max(0, min(cnt[i], cap_img));
    }
    s_off[nv] = o;
    s_nv = nv;
  }
  __syncthreads();
  const int nv = s_nv, first = ctl[1];
  for (int i = 0; i < nv; ++i) {
    const long long o = s_off[i];
    const int n = (int)(s_off[i + 1] - o);
    const float* src = rows + (size_t)i * cap_img * 6;
    for (int e = tid; e < n * 6; e += 256)
      if (o + e / 6 < rec_cap) rec_rows[(size_t)o * 6 + e] = src[e];
    for (int j = tid; j < n; j += 256)
      if (o + j < rec_cap) rec_win[o + j] = first + i;
  }
  if (tid == 0) {
    const long long total = s_off[nv];
    *rec_count = (int)(total > 0x7fffffffLL ? 0x7fffffffLL : total);
    if (total > rec_cap) *rec_overflow = 1;
  }
}

// The append of a bank of sessions (AudioDetector.open_bank): the same scan, order and clamping; the rows of image i get the session
// and the window index the group's tables name for it, win_sess[i] and win_idx[i], in place of first_window + i.
__global__ __launch_bounds__(256) void det_record_append_bank_kernel(const float* __restrict__ rows, const int* __restrict__ cnt, int B,
                                                                     int cap_img, const int* __restrict__ n_valid,
                                                                     const int* __restrict__ win_sess, const int* __restrict__ win_idx,
                                                                     float* __restrict__ rec_rows, int* __restrict__ rec_win,
                                                                     int* __restrict__ rec_sess, int rec_cap,
                                                                     int* __restrict__ rec_count, int* __restrict__ rec_overflow) {
  __shared__ long long s_off[DR_BMAX + 1];
  __shared__ int s_nv;
  const int tid = threadIdx.x;
  if (tid == 0) {
    const int nv = max(0, min(*n_valid, B));
    long long o = max(*rec_count, 0);
    for (int i = 0; i < nv; ++i) {
      s_off[i] = o;
      o += max(0, min(cnt[i], cap_img));
    }
    s_off[nv] = o;
    s_nv = nv;
  }
  __syncthreads();
  const int nv = s_nv;
  for (int i = 0; i < nv; ++i) {
    const long long o = s_off[i];
    const int n = (int)(s_off[i + 1] - o);
    const int ws = win_sess[i], wi = win_idx[i];
    const float* src = rows + (size_t)i * cap_img * 6;
    for (int e = tid; e < n * 6; e += 256)
      if (o + e / 6 < rec_cap) rec_rows[(size_t)o * 6 + e] = src[e];
    for (int j = tid; j < n; j += 256)
      if (o + j < rec_cap) {
        rec_win[o + j] = wi;
        rec_sess[o + j] = ws;
      }
  }
  if (tid == 0) {
    const long long total = s_off[nv];
    *rec_count = (int)(total > 0x7fffffffLL ? 0x7fffffffLL : total);
    if (total > rec_cap) *rec_overflow = 1;
  }
}

extern "C" int mmd_det_record_append(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, float* rec_rows, int* rec_win,
                                     int rec_cap, int* rec_count, int* rec_overflow, hipStream_t stream) {
  if (!rows || !cnt || !ctl || !rec_rows || !rec_win || !rec_count || !rec_overflow) return MMD_EINVAL;
  if (B <= 0 || B > DR_BMAX || cap_img <= 0 || rec_cap <= 0 || (long long)cap_img * 6 > 0x7fffffffLL) return MMD_EINVAL;
  hipLaunchKernelGGL(det_record_append_kernel, dim3(1), dim3(256), 0, stream, rows, cnt, B, cap_img, ctl, rec_rows, rec_win, rec_cap,
                     rec_count, rec_overflow);
  return mmd_check_launch();
}

extern "C" int mmd_det_record_append_bank(const float* rows, const int* cnt, int B, int cap_img, const int* n_valid, const int* win_sess,
                                          const int* win_idx, float* rec_rows, int* rec_win, int* rec_sess, int rec_cap, int* rec_count,
                                          int* rec_overflow, hipStream_t stream) {
  if (!rows || !cnt || !n_valid || !win_sess || !win_idx || !rec_rows || !rec_win || !rec_sess || !rec_count || !rec_overflow)
    return MMD_EINVAL;
  if (B <= 0 || B > DR_BMAX || cap_img <= 0 || rec_cap <= 0 || (long long)cap_img * 6 > 0x7fffffffLL) return MMD_EINVAL;
  hipLaunchKernelGGL(det_record_append_bank_kernel, dim3(1), dim3(256), 0, stream, rows, cnt, B, cap_img, n_valid, win_sess, win_idx,
                     rec_rows, rec_win, rec_sess, rec_cap, rec_count, rec_overflow);
  return mmd_check_launch();
}
