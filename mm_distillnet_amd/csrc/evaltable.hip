// The last stage of the device evaluation: the AP / CD table of an evaluation record, behind a stable device-wide radix sort - CDNA4 / gfx950.
//   ap_per_class / compute_ap ............ src/utils/utils.py:1188-1280
//   AP@0.5 / AP@0.75 / AP@Ave / CD table . src/utils/utils.py:2096-2181
// as mm_distillnet_amd/metrics.py (table_from_stats) restates them, with ONE difference: predictions of equal score are ranked in record
// order (a stable sort), where the host's np.argsort(-conf) leaves their order to the sorting algorithm.
//
// (a) mmd_sort_desc_f32: perm = indices by (class ascending,) key descending, index ascending.  LSD radix sort, 8-bit digits: four passes over
//     the order-preserving transform of the key (st_key_bits: descending floats -> ascending unsigned, -0 = +0, every NaN = the last value),
//     then one over the class.  A pass is three launches:
//       st_count_kernel ... one block per tile of ST_TILE items: the tile's 256-bin digit counts -> table[block][256]
//       st_scan_kernel .... ONE block: exclusive scan of the table in digit-major order (digit 0 of every block, digit 1 of every block, ...),
//                           in place: table[block][d] becomes the global position of the block's first item of digit d
//       st_scatter_kernel . one block per tile: every item goes to table[block][d] + its rank among the tile's items of digit d
//     The rank is stable.  A tile is ST_CHUNKS runs of 64 consecutive items, one run per wave instruction ("chunk"; a wave owns every fourth
//     chunk).  Within a chunk eight __ballot (64 bits wide) split the lanes by digit (st_split): the rank is the number of lower lanes of the
//     same digit, the chunk's count of a digit is written to LDS by its first lane - one writer per (chunk, digit), no atomics.  Thread d
//     then scans digit d over the chunks in order.  Counts and scatter compute the same digits from the same, unmodified input (the buffers
//     ping-pong inside ws), so the positions are a permutation of 0 .. n-1; the store is bounds-checked all the same.
//     No block waits for another block: every inter-block dependency is a kernel boundary.  No global atomics (the class check's sticky
//     status flag apart, which orders nothing).
// (b) mmd_eval_table: et_prep_kernel (ground truth per class) -> the sort with cls = label, so each class is one contiguous segment ->
//     et_bounds_kernel (segment ends) -> et_ap_kernel, one block per (class, IoU threshold) -> et_final_kernel (means, CD averages, out).
//     The AP arithmetic is float64 throughout, operation for operation ap_per_class / compute_ap; only the order of the final sum differs.
#include "common.h"
// the float32 quotients of the central distances are rounded as numpy rounds them: no contraction, IEEE division (see evalstats.hip)
#pragma clang fp contract(off)

#define ST_THREADS 256
#define ST_ROUNDS 8
#define ST_TILE (ST_THREADS * ST_ROUNDS)      // items per block: 32 chunks x 256 counters = 32 KB of LDS, 4 blocks per CU stay resident
#define ST_CHUNKS (ST_TILE / 64)
#define ST_SCAN_THREADS 1024
#define ET_NT 9
#define ET_THREADS 1024

// descending float order as ascending unsigned order; integer tests, so no denormal mode can touch it
__device__ __forceinline__ unsigned st_key_bits(float x) {
  unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;      // NaN: behind everything (only the pattern 0xffffffff, a NaN, maps here)
  if ((u & 0x7fffffffu) == 0u) u = 0u;                           // -0.0 -> +0.0
  return ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
}
// a class id: an integer 0 .. 255 stored as float, or -1
__device__ __forceinline__ int et_class(float v) { return (v >= 0.f && v <= 255.f && v == floorf(v)) ? (int)v : -1; }

// Lanes of one wave by 8-bit digit: rank = lower valid lanes of the same digit, count = all of them.  Every lane of the wave calls it.
__device__ __forceinline__ void st_split(int d, bool valid, int& rank, int& count) {
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1;
    const unsigned long long m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  const int lane = threadIdx.x & 63;
  rank = __popcll(peers & ((1ull << lane) - 1ull));
  count = __popcll(peers);
}

// MODE 0: first key pass (float keys, index = position); 1: later key pass (transformed keys and indices of the pass before); 2: class pass
struct SortPass {
  const float* key; long long kstride;
  const float* cls; long long cstride;
  const unsigned* kin; const int* iin;
  unsigned* kout; int* iout;      // kout null: the keys are not needed behind this pass
  int* table; int* status; long long n; int shift;
};

// The tile's items into registers, their per-chunk digit counts into s_cnt.  dr = digit | rank within the chunk << 8, or -1 behind n.
template <int MODE>
__device__ __forceinline__ bool st_tile(const SortPass& a, int (*s_cnt)[256], unsigned (&k)[ST_ROUNDS], int (&idx)[ST_ROUNDS], int (&dr)[ST_ROUNDS]) {
  const int tid = threadIdx.x;
  for (int e = tid; e < ST_CHUNKS * 256; e += ST_THREADS) (&s_cnt[0][0])[e] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * ST_TILE;
  bool bad = false;
#pragma unroll
  for (int r = 0; r < ST_ROUNDS; ++r) {
    const long long pos = base + r * ST_THREADS + tid;
    const bool valid = pos < a.n;
    int d = 0;
    k[r] = 0u; idx[r] = 0;
    if (valid) {
      if (MODE == 0) { idx[r] = (int)pos; k[r] = st_key_bits(a.key[pos * a.kstride]); }
      else { idx[r] = a.iin[pos]; if (MODE == 1) k[r] = a.kin[pos]; }
      if (MODE == 2) {
        // (an index is never trusted into an address: the passes before wrote a permutation of 0 .. n-1)
        const int c = (unsigned)idx[r] < (unsigned long long)a.n ? et_class(a.cls[(long long)idx[r] * a.cstride]) : -1;
        bad |= c < 0;
        d = c < 0 ? 0 : c;
      } else d = (int)((k[r] >> a.shift) & 255u);
    }
    int rank, count;
    st_split(d, valid, rank, count);
    if (valid && rank == 0) s_cnt[r * (ST_THREADS / 64) + (tid >> 6)][d] = count;
    dr[r] = valid ? (d | (rank << 8)) : -1;
  }
  __syncthreads();
  return bad;
}

template <int MODE>
__global__ __launch_bounds__(ST_THREADS) void st_count_kernel(SortPass a) {
  __shared__ int s_cnt[ST_CHUNKS][256];
  unsigned k[ST_ROUNDS]; int idx[ST_ROUNDS], dr[ST_ROUNDS];
  const bool bad = st_tile<MODE>(a, s_cnt, k, idx, dr);
  if (MODE == 2 && bad) atomicOr(a.status, 1);
  const int d = threadIdx.x;
  int sum = 0;
#pragma unroll
  for (int c = 0; c < ST_CHUNKS; ++c) sum += s_cnt[c][d];
  a.table[(size_t)blockIdx.x * 256 + d] = sum;
}

// One block.  Thread (g, d) owns digit d of a quarter of the blocks.
__global__ __launch_bounds__(ST_SCAN_THREADS) void st_scan_kernel(int* table, int nblk) {
  __shared__ int s_part[4][256];
  __shared__ int s_excl[256];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, g = tid >> 8, d = tid & 255, lane = tid & 63;
  const int per = (nblk + 3) / 4, b0 = min(nblk, g * per), b1 = min(nblk, b0 + per);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += table[(size_t)b * 256 + d];
  s_part[g][d] = sum;
  __syncthreads();
  int tot = 0, inc = 0;
  if (tid < 256) {      // exclusive scan of the 256 digit totals: inclusive within the wave, then the waves in front
    tot = s_part[0][d] + s_part[1][d] + s_part[2][d] + s_part[3][d];
    inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) s_wave[tid >> 6] = inc;
  }
  __syncthreads();
  if (tid < 256) {
    int front = 0;
    for (int w = 0; w < (tid >> 6); ++w) front += s_wave[w];
    s_excl[d] = front + inc - tot;
  }
  __syncthreads();
  int run = s_excl[d];
  for (int q = 0; q < g; ++q) run += s_part[q][d];
  for (int b = b0; b < b1; ++b) {
    const size_t e = (size_t)b * 256 + d;
    const int v = table[e];
    table[e] = run;
    run += v;
  }
}

template <int MODE>
__global__ __launch_bounds__(ST_THREADS) void st_scatter_kernel(SortPass a) {
  __shared__ int s_cnt[ST_CHUNKS][256];
  __shared__ int s_base[256];
  unsigned k[ST_ROUNDS]; int idx[ST_ROUNDS], dr[ST_ROUNDS];
  st_tile<MODE>(a, s_cnt, k, idx, dr);
  const int tid = threadIdx.x;
  int run = 0;
#pragma unroll
  for (int c = 0; c < ST_CHUNKS; ++c) { const int v = s_cnt[c][tid]; s_cnt[c][tid] = run; run += v; }
  s_base[tid] = a.table[(size_t)blockIdx.x * 256 + tid];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < ST_ROUNDS; ++r) {
    if (dr[r] < 0) continue;
    const int d = dr[r] & 255;
    const long long dst = (long long)s_base[d] + s_cnt[r * (ST_THREADS / 64) + (tid >> 6)][d] + (dr[r] >> 8);
    if (dst < 0 || dst >= a.n) continue;      // cannot happen (see the head of the file); an index is never trusted into a store
    a.iout[dst] = idx[r];
    if (MODE != 2 && a.kout) a.kout[dst] = k[r];
  }
}

static inline long long st_blocks(long long n) { return (n + ST_TILE - 1) / ST_TILE; }
static inline long long et_al(long long bytes) { return (bytes + 255) / 256 * 256; }
static inline bool et_misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
// ws: table int[blocks][256] | keys unsigned[n] x 2 | indices int[n] x 2
static long long st_ws_bytes(long long n) { return et_al(st_blocks(n) * 1024) + 4 * et_al(n * 4) + 256; }

template <int MODE>
static void st_pass(const SortPass& a, hipStream_t stream) {
  const int nblk = (int)st_blocks(a.n);
  hipLaunchKernelGGL(st_count_kernel<MODE>, dim3(nblk), dim3(ST_THREADS), 0, stream, a);
  hipLaunchKernelGGL(st_scan_kernel, dim3(1), dim3(ST_SCAN_THREADS), 0, stream, a.table, nblk);
  hipLaunchKernelGGL(st_scatter_kernel<MODE>, dim3(nblk), dim3(ST_THREADS), 0, stream, a);
}

// 0 < n < 2^31, pointers checked by the callers; key / cls are read at [i * stride]
static void st_sort(const float* key, long long kstride, const float* cls, long long cstride, long long n, int* perm_out, void* ws,
                    int* status, hipStream_t stream) {
  char* w = static_cast<char*>(ws);
  int* table = reinterpret_cast<int*>(w); w += et_al(st_blocks(n) * 1024);
  unsigned* kb[2]; int* ib[2];
  for (int i = 0; i < 2; ++i) { kb[i] = reinterpret_cast<unsigned*>(w); w += et_al(n * 4); }
  for (int i = 0; i < 2; ++i) { ib[i] = reinterpret_cast<int*>(w); w += et_al(n * 4); }
  SortPass a{key, kstride, cls, cstride, nullptr, nullptr, kb[0], ib[0], table, status, n, 0};
  st_pass<0>(a, stream);
  for (int p = 1; p < 4; ++p) {
    a.kin = kb[(p - 1) & 1]; a.iin = ib[(p - 1) & 1];
    a.kout = p < 3 ? kb[p & 1] : nullptr;
    a.iout = (p == 3 && !cls) ? perm_out : ib[p & 1];
    a.shift = 8 * p;
    st_pass<1>(a, stream);
  }
  if (cls) {
    a.kin = nullptr; a.iin = ib[1]; a.kout = nullptr; a.iout = perm_out; a.shift = 0;
    st_pass<2>(a, stream);
  }
}

extern "C" int mmd_sort_tile(void) { return ST_TILE; }

// bytes of mmd_sort_desc_f32's ws for n keys; -22 for n < 0, n >= 2^31 or a size that does not fit an int
extern "C" int mmd_sort_desc_ws_bytes(long long n) {
  if (n < 0 || n > 0x7fffffffll) return MMD_EINVAL;
  const long long b = st_ws_bytes(n);
  return b > 0x7fffffffll ? MMD_EINVAL : (int)b;
}

extern "C" int mmd_sort_desc_f32(const float* key, const float* cls, long long n, int* perm_out, void* ws, int* status, hipStream_t stream) {
  if (n < 0 || n > 0x7fffffffll || mmd_sort_desc_ws_bytes(n) < 0) return MMD_EINVAL;
  if (!ws || !status || et_misaligned(ws, 16) || et_misaligned(status, 4)) return MMD_EINVAL;
  if (et_misaligned(key, 4) || et_misaligned(cls, 4) || et_misaligned(perm_out, 4)) return MMD_EINVAL;
  if (n == 0) return MMD_OK;
  if (!key || !perm_out) return MMD_EINVAL;
  st_sort(key, 1, cls, 1, n, perm_out, ws, status, stream);
  return mmd_check_launch();
}

// ---- the table -------------------------------------------------------------------------------------------------------------------------
struct EtArgs {
  const float* rows; const int* tp; long long n_rows;      // rows [n_rows, 2] = (score, class)
  const float* cd; long long n_img;
  const float* gt; long long n_gt;
  float image_size;
  int* gtcount; int* seg_lo; int* seg_hi;      // [256] each
  double* ap;                                  // [256][ET_NT]
  double* pr;                                  // [256][2]: precision, recall at threshold 0
  int* perm; double* out; int* status;
};

// One block: ground-truth boxes per class, the segment table cleared.  A wave adds each digit once per 64 boxes (st_split).
__global__ __launch_bounds__(ET_THREADS) void et_prep_kernel(EtArgs a) {
  __shared__ int s_h[256];
  const int tid = threadIdx.x;
  if (tid < 256) s_h[tid] = 0;
  __syncthreads();
  bool bad = false;
  for (long long b = 0; b < a.n_gt; b += ET_THREADS) {
    const long long i = b + tid;
    const bool valid = i < a.n_gt;
    const int c = valid ? et_class(a.gt[i]) : 0;
    bad |= c < 0;
    int rank, count;
    st_split(c < 0 ? 0 : c, valid && c >= 0, rank, count);
    if (valid && c >= 0 && rank == 0) atomicAdd(&s_h[c], count);
  }
  if (bad) atomicOr(a.status, 1);
  __syncthreads();
  if (tid < 256) { a.gtcount[tid] = s_h[tid]; a.seg_lo[tid] = 0; a.seg_hi[tid] = 0; }
}

// class / true-positive mask of the row at sorted position pos (-1 / 0 for an index outside the record: never trusted into an address)
__device__ __forceinline__ int et_class_at(const EtArgs& a, long long pos) {
  const int p = a.perm[pos];
  return (unsigned)p < (unsigned long long)a.n_rows ? et_class(a.rows[2 * (long long)p + 1]) : -1;
}
__device__ __forceinline__ int et_tp_at(const EtArgs& a, long long pos) {
  const int p = a.perm[pos];
  return (unsigned)p < (unsigned long long)a.n_rows ? a.tp[p] : 0;
}

// perm is sorted by class: the positions where the class changes are the segments' ends
__global__ __launch_bounds__(256) void et_bounds_kernel(EtArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows) return;
  const int c = et_class_at(a, i);
  if (c < 0) return;      // the sort has set *status
  if (i == 0 || et_class_at(a, i - 1) != c) a.seg_lo[c] = (int)i;
  if (i == a.n_rows - 1 || et_class_at(a, i + 1) != c) a.seg_hi[c] = (int)(i + 1);
}

// Block (c, k): AP of class c at threshold k.  With i the rank within the segment and q = m - 1 - i the position from its end:
//   hits_i = total - (true positives at ranks > i) - an exclusive prefix count in q order;
//   envelope_i = max_{j >= i} p_j - an inclusive prefix maximum in q order.
// The segment is walked from its end in tiles of ET_THREADS; `seen` and `runmax` carry both across tiles.
__global__ __launch_bounds__(ET_THREADS) void et_ap_kernel(EtArgs a) {
  __shared__ int s_wc[ET_THREADS / 64];
  __shared__ double s_wm[ET_THREADS / 64];
  __shared__ double s_ws[ET_THREADS / 64];
  constexpr int NW = ET_THREADS / 64;
  const int c = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n_c = a.gtcount[c];
  const long long lo = min((long long)max(a.seg_lo[c], 0), a.n_rows), hi = min((long long)max(a.seg_hi[c], 0), a.n_rows);
  const long long m = n_c > 0 && hi > lo ? hi - lo : 0;
  if (m == 0) {      // not in the ground truth (ignored), or nobody predicted it: 0
    if (tid == 0) { a.ap[c * ET_NT + k] = 0.0; if (k == 0) { a.pr[2 * c] = 0.0; a.pr[2 * c + 1] = 0.0; } }
    return;
  }
  // ---- total hits
  int cnt = 0;
  for (long long i = tid; i < m; i += ET_THREADS) cnt += (et_tp_at(a, lo + i) >> k) & 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) s_wc[wave] = cnt;
  __syncthreads();
  long long total = 0;
  for (int w = 0; w < NW; ++w) total += s_wc[w];
  __syncthreads();
  // ---- the walk
  const double den = (double)n_c + 1e-16;
  long long seen = 0;
  double runmax = 0.0, acc = 0.0;
  for (long long q0 = 0; q0 < m; q0 += ET_THREADS) {
    const long long q = q0 + tid, i = m - 1 - q;
    const bool valid = q < m;
    const bool hit = valid && ((et_tp_at(a, lo + i) >> k) & 1);
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_wc[wave] = __popcll(bal);
    __syncthreads();
    int front = 0, tile = 0;
    for (int w = 0; w < NW; ++w) { const int v = s_wc[w]; tile += v; if (w < wave) front += v; }
    const long long hits = total - seen - front - __popcll(bal & ((1ull << lane) - 1ull));
    double e = valid ? (double)hits / (double)(i + 1) : 0.0;      // precision is >= 0: 0 is neutral for the maximum
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(e, o, 64); if (lane >= o) e = fmax(e, t); }
    if (lane == 63) s_wm[wave] = e;
    __syncthreads();
    double carry = runmax, tmax = runmax;
    for (int w = 0; w < NW; ++w) { const double v = s_wm[w]; tmax = fmax(tmax, v); if (w < wave) carry = fmax(carry, v); }
    if (hit) acc += ((double)hits / den - (double)(hits - 1) / den) * fmax(e, carry);
    seen += tile; runmax = tmax;
    __syncthreads();
  }
  acc = wave_sum_d(acc);
  if (lane == 0) s_ws[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += s_ws[w];
    a.ap[c * ET_NT + k] = s;
    if (k == 0) { a.pr[2 * c] = (double)total / (double)m; a.pr[2 * c + 1] = (double)total / den; }
  }
}

// One block, thread = class id: the means over the ground-truth classes, the CD averages, every element of out.
__global__ __launch_bounds__(256) void et_final_kernel(EtArgs a) {
  __shared__ double s_mean[ET_NT];
  __shared__ double s_cd[4][3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n_c = a.gtcount[tid];
  const int ncls = __syncthreads_count(n_c > 0);
  if (tid < ET_NT) {
    double s = 0.0;
    for (int c = 0; c < 256; ++c) if (a.gtcount[c] > 0) s += a.ap[c * ET_NT + tid];
    s_mean[tid] = a.n_rows == 0 ? 0.0 : s / (double)ncls;      // no ground truth at all: 0 / 0, the NaN of the host's empty mean
  }
  double sx = 0.0, sy = 0.0, sn = 0.0;
  for (long long i = tid; i < a.n_img; i += 256) {
    const float nb = a.cd[3 * i + 2];
    if (nb > 0.f) { sx += (double)(a.cd[3 * i] / nb / a.image_size); sy += (double)(a.cd[3 * i + 1] / nb / a.image_size); sn += 1.0; }
  }
  sx = wave_sum_d(sx); sy = wave_sum_d(sy); sn = wave_sum_d(sn);
  if (lane == 0) { s_cd[wave][0] = sx; s_cd[wave][1] = sy; s_cd[wave][2] = sn; }
  __syncthreads();
  double* row = a.out + 16 + 8 * tid;
  const bool present = n_c > 0;
  const double p = present ? a.pr[2 * tid] : 0.0, r = present ? a.pr[2 * tid + 1] : 0.0;
  row[0] = present ? 1.0 : 0.0;
  row[1] = (double)n_c;
  row[2] = present ? (double)max(0, a.seg_hi[tid] - a.seg_lo[tid]) : 0.0;
  row[3] = p; row[4] = r;
  row[5] = present ? a.ap[tid * ET_NT] : 0.0;
  row[6] = present ? 2.0 * p * r / (p + r + 1e-16) : 0.0;
  row[7] = 0.0;
  if (tid == 0) {
    double ave = 0.0;
    for (int k = 0; k < ET_NT; ++k) { a.out[k] = s_mean[k]; ave += s_mean[k]; }
    a.out[9] = ave / (double)ET_NT * 100.0;
    a.out[10] = s_mean[0] * 100.0;
    a.out[11] = s_mean[5] * 100.0;
    const double n = s_cd[0][2] + s_cd[1][2] + s_cd[2][2] + s_cd[3][2];
    // no prediction in the record: the reference's sentinel row, 100 (x 100)
    a.out[12] = a.n_rows == 0 ? 10000.0 : (s_cd[0][0] + s_cd[1][0] + s_cd[2][0] + s_cd[3][0]) / n * 100.0;
    a.out[13] = a.n_rows == 0 ? 10000.0 : (s_cd[0][1] + s_cd[1][1] + s_cd[2][1] + s_cd[3][1]) / n * 100.0;
    a.out[14] = (double)ncls;
    a.out[15] = 0.0;
  }
}

// ws: gtcount | seg_lo | seg_hi int[256] each | ap double[256][9] | pr double[256][2] | perm int[n_rows] | the sort's ws
#define ET_HEAD_BYTES (3 * 1024 + 256 * ET_NT * 8 + 256 * 2 * 8)
extern "C" int mmd_eval_table_ws_bytes(long long n_rows, long long n_gt) {
  if (n_rows < 0 || n_gt < 0 || n_rows > 0x7fffffffll || n_gt > 0x7fffffffll) return MMD_EINVAL;
  const long long b = et_al(ET_HEAD_BYTES) + et_al(n_rows * 4) + st_ws_bytes(n_rows);
  return b > 0x7fffffffll ? MMD_EINVAL : (int)b;
}

extern "C" int mmd_eval_table(const float* score_label, const int* tp, long long n_rows, const float* cd, long long n_img, const float* gt,
                              long long n_gt, float image_size, double* out, void* ws, int* status, hipStream_t stream) {
  if (n_rows < 0 || n_img < 0 || n_gt < 0 || n_img > 0x7fffffffll || mmd_eval_table_ws_bytes(n_rows, n_gt) < 0) return MMD_EINVAL;
  if (!out || !ws || !status || et_misaligned(out, 8) || et_misaligned(ws, 16) || et_misaligned(status, 4)) return MMD_EINVAL;
  if (et_misaligned(score_label, 4) || et_misaligned(tp, 4) || et_misaligned(cd, 4) || et_misaligned(gt, 4)) return MMD_EINVAL;
  if ((n_rows > 0 && (!score_label || !tp)) || (n_img > 0 && !cd) || (n_gt > 0 && !gt)) return MMD_EINVAL;
  char* w = static_cast<char*>(ws);
  EtArgs a{score_label, tp, n_rows, cd, n_img, gt, n_gt, image_size};
  a.gtcount = reinterpret_cast<int*>(w); a.seg_lo = a.gtcount + 256; a.seg_hi = a.gtcount + 512;
  a.ap = reinterpret_cast<double*>(w + 3 * 1024); a.pr = a.ap + 256 * ET_NT;
  w += et_al(ET_HEAD_BYTES);
  a.perm = reinterpret_cast<int*>(w); w += et_al(n_rows * 4);
  a.out = out; a.status = status;
  hipLaunchKernelGGL(et_prep_kernel, dim3(1), dim3(ET_THREADS), 0, stream, a);
  if (n_rows > 0) {
    st_sort(score_label, 2, score_label + 1, 2, n_rows, a.perm, w, status, stream);
    hipLaunchKernelGGL(et_bounds_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, stream, a);
  }
  hipLaunchKernelGGL(et_ap_kernel, dim3(256, ET_NT), dim3(ET_THREADS), 0, stream, a);
  hipLaunchKernelGGL(et_final_kernel, dim3(1), dim3(256), 0, stream, a);
  return mmd_check_launch();
}
