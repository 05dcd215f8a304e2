// Evaluation metrics (the reference's MetricLogger on torchmetrics: ROC at T thresholds, AUROC, accuracy) from integer counts.
// include/wvn_hip.h "evaluation metrics" is the interface, tests/metrics_ref.py the definition, DESIGN.md section 4 "Evaluation
// metrics" the LDS budget and the reasons.  Compiled with -ffp-contract=off: the binned AUROC is a fixed sequence of fp64 operations.
//
//   metric_accumulate_kernel      the fused pixel pass: up to 2 scores x 2 targets over [B][H][W], dense or gathered through seg on
//                                 load -> the pair histograms, confusion matrices and counters, per-segment class counts
//   metric_curve_kernel           one pair state -> fpr / tpr / thresholds (ascending fpr), binned AUROC, accuracy, P, N
//   metric_auroc_weighted_kernel  sorted weighted entries -> the Mann-Whitney statistic with tie groups, exact in int64
//
// The pixel pass: grid (x, n_scores [+ 1]), a workgroup owns one contiguous run of pixels.  A slice (blockIdx.y) owns ONE score and
// all of its targets: the bin search against the threshold table is done once per pixel and score, the workgroup's histogram
// [T + 1][n_targets][2] of 32-bit counters lives in LDS (80 KB at T = 5000 with two targets: two workgroups of 512 threads per CU;
// 131 KB at T = 8192: one), the slices re-read the pixels from the cache.  A workgroup sees fewer than 2^31 pixels, so a 32-bit
// counter cannot overflow.  Real frames put whole regions into one bin: before it touches LDS a wave merges the lanes that share
// the first active lane's (bin, classes) key into one add of their count, twice (a region and its neighbour), and only what is
// left adds lane by lane.  The flush is one 64-bit atomic per non-empty counter and workgroup.  Where per-segment counts are
// wanted, one more slice takes them: the same LDS as a window of segment rows from the first row of the frame its run begins in
// (a run is a fraction of a frame), rows outside the window added to global memory directly (one global atomic per merged wave group
// is a wave instruction with a single lane at work: far slower than the rest of the pass).  Segment ids are read as int32 or int64.
// Sums of integers: the result depends on neither geometry nor arrival order.
#include "../../include/wvn_hip.h"

#include "common.h"
#include "wvn_internal.h"

namespace {

constexpr int MA_THREADS = 512;
constexpr int MA_PIX = 4;          // consecutive pixels per thread and round
constexpr int MA_MAX_BLOCKS = 512; // per slice: two resident workgroups on each of 256 CUs
constexpr int MA_SEG_WINDOW_WORDS = 8192;   // at least this much LDS where per-segment counts are taken: a window of >= 2048 rows
constexpr int MA_TAIL = 16;        // LDS words behind the histogram: per target {cm[4], n_nan, n_ignored, n_out_of_range, -}
constexpr int MC_THREADS = 1024;
constexpr int MW_ITEMS = 4;

struct MaArgs {
  wvn_metric_desc d;
  unsigned npix, plane;
  int any_seg;   // a per-segment source is in use: pixels with an id outside the frame's segments are skipped
  int lds_words; // dynamic LDS of the launch
  unsigned chunk; // pixel groups per workgroup (a multiple of MA_THREADS): a workgroup owns one contiguous run of pixels
};

// k(p) = #{t : th[t] <= p}: the uniform-table guess ...
__device__ inline int ma_guess(float p, int T) {
  const float x = __fmul_rn(p, (float)(T - 1));
  if (!(x > 0.f)) return 0;
  if (x >= (float)T) return T;
  return (int)x + 1;
}
// ... corrected against the table itself (both loops end: g stays in [0, T])
__device__ inline int ma_bin(float p, int g, const float* __restrict__ th, int T) {
  while (g < T && th[g] <= p) ++g;
  while (g > 0 && th[g - 1] > p) --g;
  return g;
}

// class of a raw target word: 0 negative, 1 positive, 2 skipped
__device__ inline int ma_class(uint32_t w, int dtype, int has_ign, int ign) {
  long long v;
  if (dtype == WVN_METRIC_F32) {
    const float f = __uint_as_float(w);
    if (!(__builtin_fabsf(f) < 2.0e9f)) return 2;   // NaN, inf, and values no label takes
    v = (long long)f;                               // truncation toward zero
  } else if (dtype == WVN_METRIC_I32) {
    v = (long long)(int)w;
  } else {
    v = (long long)(w & 255u);
  }
  if (has_ign && v == (long long)ign) return 2;
  return v == 0 ? 0 : (v == 1 ? 1 : 2);
}

__device__ inline uint32_t ma_load1(const void* base, int esize, long long i) {
  return esize == 1 ? (uint32_t)((const unsigned char*)base)[i] : ((const uint32_t*)base)[i];
}

// MA_PIX consecutive elements from p0 (nv of them exist): one vector load where the address allows it
__device__ inline void ma_load4(const void* base, int esize, long long p0, int nv, uint32_t (&w)[MA_PIX]) {
#pragma unroll
  for (int j = 0; j < MA_PIX; ++j) w[j] = 0u;
  if (esize == 1) {
    const unsigned char* p = (const unsigned char*)base + p0;
    if (nv == MA_PIX && ((uintptr_t)p & 3) == 0) {
      const uint32_t v = *(const uint32_t*)p;
#pragma unroll
      for (int j = 0; j < MA_PIX; ++j) w[j] = (v >> (8 * j)) & 255u;
    } else {
#pragma unroll
      for (int j = 0; j < MA_PIX; ++j)
        if (j < nv) w[j] = p[j];
    }
  } else {
    const uint32_t* p = (const uint32_t*)base + p0;
    if (nv == MA_PIX && ((uintptr_t)p & 15) == 0) {
      const u32x4_t v = *(const u32x4_t*)p;
#pragma unroll
      for (int j = 0; j < MA_PIX; ++j) w[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < MA_PIX; ++j)
        if (j < nv) w[j] = p[j];
    }
  }
}

// the same for 64-bit segment ids
__device__ inline void ma_load4_i64(const void* base, long long p0, int nv, long long (&w)[MA_PIX]) {
  const long long* p = (const long long*)base + p0;
  if (nv == MA_PIX && ((uintptr_t)p & 15) == 0) {
    const u32x4_t a = ((const u32x4_t*)p)[0], b = ((const u32x4_t*)p)[1];
    w[0] = (long long)(((unsigned long long)a[1] << 32) | a[0]);
    w[1] = (long long)(((unsigned long long)a[3] << 32) | a[2]);
    w[2] = (long long)(((unsigned long long)b[1] << 32) | b[0]);
    w[3] = (long long)(((unsigned long long)b[3] << 32) | b[2]);
  } else {
#pragma unroll
    for (int j = 0; j < MA_PIX; ++j) w[j] = j < nv ? p[j] : 0;
  }
}

// Every lane of the wave calls this together.  The lanes that share the key of the first active lane become ONE add of their
// count, made by that lane; twice; what is left adds for itself.
template <typename K, typename F>
__device__ inline void ma_wave_add(K key, bool active, F add) {
  const int lane = threadIdx.x & (WVN_WAVE - 1);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;
    const int src = __ffsll((long long)act) - 1;
    const K k0 = __shfl(key, src, WVN_WAVE);
    const bool mine = active && key == k0;
    const unsigned long long m = __ballot(mine);
    if (lane == src) add(k0, (unsigned)__popcll(m));
    active = active && !mine;
  }
  if (active) add(key, 1u);
}

__device__ inline int ma_esize(int dtype) { return dtype == WVN_METRIC_U8 ? 1 : 4; }

extern __shared__ unsigned ma_lds[];

__global__ __launch_bounds__(MA_THREADS) void metric_accumulate_kernel(const MaArgs a) {
  const wvn_metric_desc& d = a.d;
  // slices 0 .. n_scores - 1: one score each; slice n_scores (only with seg_counts): the per-segment class counts
  const bool seg_slice = (int)blockIdx.y == d.n_scores;
  const int s = seg_slice ? 0 : (int)blockIdx.y;
  const int NT = d.n_targets, T = d.T;
  const int nctr = (T + 1) * NT * 2;
  for (int i = threadIdx.x; i < a.lds_words; i += MA_THREADS) ma_lds[i] = 0u;
  __syncthreads();

  const float* __restrict__ th = d.thresholds;
  const float* sc_base = d.score[s];
  const bool sc_seg = d.score_kind[s] == WVN_METRIC_PER_SEGMENT && !seg_slice;
  const long long sc_stride = d.score_stride[s];
  const bool have_seg = d.seg != nullptr;
  const bool skip_unknown = a.any_seg && !seg_slice;
  const float tau = d.tau;
  unsigned* const hist = ma_lds;
  int* const segc = d.seg_counts;

  int cnt[2][7];   // per target: cm[c][pred] (4), n_nan, n_ignored, n_out_of_range
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 7; ++q) cnt[t][q] = 0;

  const unsigned ngroups = (a.npix + MA_PIX - 1) / MA_PIX;
  const unsigned gfirst = blockIdx.x * a.chunk;
  const unsigned gend = gfirst + a.chunk < ngroups ? gfirst + a.chunk : ngroups;
  // The segment slice keeps the counts of a window of rows in LDS: [wb, wb + wrows) from the first row of the frame this
  // workgroup's run begins in (a run is a fraction of a frame; a row outside the window adds to global memory directly).
  long long wb = 0;
  const long long wrows = a.lds_words / (NT * 2);
  if (seg_slice && gfirst < ngroups) {
    const unsigned b0 = (unsigned)((long long)gfirst * MA_PIX / a.plane);
    wb = d.seg_off ? d.seg_off[b0] : (long long)b0 * d.S;
  }
  for (unsigned g0 = gfirst; g0 < gend; g0 += MA_THREADS) {   // (the same trip count for every lane)
    const unsigned g = g0 + threadIdx.x;
    const bool in = g < gend;
    const long long p0 = (long long)g * MA_PIX;
    int nv = 0;
    if (in) nv = a.npix - (unsigned)p0 < (unsigned)MA_PIX ? (int)(a.npix - (unsigned)p0) : MA_PIX;
    uint32_t wseg[MA_PIX], wsc[MA_PIX], wt[2][MA_PIX];
    long long sid64[MA_PIX];
#pragma unroll
    for (int j = 0; j < MA_PIX; ++j) {
      wseg[j] = wsc[j] = wt[0][j] = wt[1][j] = 0u;
      sid64[j] = 0;
    }
    unsigned b = 0, r = 0;
    if (in) {
      if (have_seg) {
        if (d.seg_bytes == 8) {
          ma_load4_i64(d.seg, p0, nv, sid64);
        } else {
          ma_load4(d.seg, 4, p0, nv, wseg);
#pragma unroll
          for (int j = 0; j < MA_PIX; ++j) sid64[j] = (long long)(int)wseg[j];
        }
        b = (unsigned)p0 / a.plane;
        r = (unsigned)p0 - b * a.plane;
      }
      if (!sc_seg && !seg_slice) ma_load4(sc_base, 4, p0, nv, wsc);
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (t < NT && d.target_kind[t] == WVN_METRIC_DENSE) ma_load4(d.target[t], ma_esize(d.target_dtype[t]), p0, nv, wt[t]);
    }
    // The rows of the four pixels, then every gather of the round, then the table look-ups: the loads of a phase are independent
    // and in flight together (the pass is bound by their latency, not by bytes).
    bool seg_ok[MA_PIX];
    long long row[MA_PIX];
#pragma unroll
    for (int j = 0; j < MA_PIX; ++j) {
      seg_ok[j] = false;
      row[j] = 0;
      if (j < nv && have_seg) {
        while (r >= a.plane) { r -= a.plane; ++b; }
        const long long sid = sid64[j];
        long long base = (long long)b * d.S;
        long long n = d.S;
        if (d.seg_off) {
          base = d.seg_off[b];
          n = d.seg_off[b + 1] - base;
        }
        seg_ok[j] = sid >= 0 && sid < n;
        row[j] = seg_ok[j] ? base + sid : 0;
        ++r;
      }
    }
    float p[MA_PIX];
    int c[MA_PIX][2];
#pragma unroll
    for (int j = 0; j < MA_PIX; ++j) {
      p[j] = 0.f;
      c[j][0] = c[j][1] = 2;
      if (j < nv && !(skip_unknown && !seg_ok[j])) {
        p[j] = sc_seg ? sc_base[row[j] * sc_stride] : __uint_as_float(wsc[j]);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (t >= NT) continue;
          const uint32_t w = d.target_kind[t] == WVN_METRIC_DENSE
                                 ? wt[t][j]
                                 : ma_load1(d.target[t], ma_esize(d.target_dtype[t]), row[j] * d.target_stride[t]);
          c[j][t] = ma_class(w, d.target_dtype[t], d.has_ignore, d.ignore_index);
        }
      }
    }
    int bin[MA_PIX];
    bool settled[MA_PIX];
    if (seg_slice) {
#pragma unroll
      for (int j = 0; j < MA_PIX; ++j) {
        bool sact = false;
        long long skey = 0;
        if (j < nv && seg_ok[j] && (c[j][0] < 2 || c[j][1] < 2)) {
          sact = true;
          skey = row[j] * 16 + (c[j][0] | (c[j][1] << 2));
        }
        ma_wave_add(skey, sact, [&](long long key, unsigned n) {
          const long long rw = key >> 4, w = rw - wb;
          const int c0 = (int)(key & 3), c1 = (int)((key >> 2) & 3);
          if (w >= 0 && w < wrows) {
            if (c0 < 2) atomicAdd(&ma_lds[(w * NT + 0) * 2 + c0], n);
            if (c1 < 2) atomicAdd(&ma_lds[(w * NT + 1) * 2 + c1], n);
          } else {
            if (c0 < 2) atomicAdd(&segc[(rw * NT + 0) * 2 + c0], (int)n);
            if (c1 < 2) atomicAdd(&segc[(rw * NT + 1) * 2 + c1], (int)n);
          }
        });
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < MA_PIX; ++j) {   // the guess is right when th[g - 1] <= p < th[g]: both neighbours in one round of loads
      const int g = ma_guess(p[j], T);
      const float lo = th[g > 0 ? g - 1 : 0], hi = th[g < T ? g : T - 1];
      bin[j] = g;
      settled[j] = (g == 0 || lo <= p[j]) && (g == T || hi > p[j]);
    }
#pragma unroll
    for (int j = 0; j < MA_PIX; ++j)
      if (!settled[j] && p[j] == p[j]) bin[j] = ma_bin(p[j], bin[j], th, T);
#pragma unroll
    for (int j = 0; j < MA_PIX; ++j) {
      int hkey = 0;
      bool hact = false;
      if (j < nv) {
        const bool nan = p[j] != p[j];
        const int pred = p[j] > tau ? 1 : 0;
        const int oor = (p[j] < 0.f || p[j] > 1.f) ? 1 : 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (t >= NT) continue;
          if (c[j][t] == 2) {
            ++cnt[t][5];
          } else if (nan) {
            ++cnt[t][4];
          } else {
            if (c[j][t] == 0) { if (pred) ++cnt[t][1]; else ++cnt[t][0]; }
            else              { if (pred) ++cnt[t][3]; else ++cnt[t][2]; }
            cnt[t][6] += oor;
          }
        }
        const int code = c[j][0] | (c[j][1] << 2);
        const bool any = c[j][0] < 2 || c[j][1] < 2;
        if (any && !nan) {
          hact = true;
          hkey = bin[j] * 16 + code;
        }
      }
      ma_wave_add(hkey, hact, [&](int key, unsigned n) {
        const int k = key >> 4, c0 = key & 3, c1 = (key >> 2) & 3;
        if (c0 < 2) atomicAdd(&hist[(k * NT + 0) * 2 + c0], n);
        if (c1 < 2) atomicAdd(&hist[(k * NT + 1) * 2 + c1], n);   // (c1 is 2 where there is one target)
      });
    }
  }

  if (seg_slice) {   // the window's counts: one atomic per non-empty counter
    __syncthreads();
    const long long words = wrows * NT * 2;
    for (long long i = threadIdx.x; i < words; i += MA_THREADS) {
      const unsigned v = ma_lds[i];
      if (v != 0u) atomicAdd(&segc[wb * NT * 2 + i], (int)v);
    }
    return;
  }
  // confusion matrices and counters: wave sums, one LDS add per wave, flushed with the histogram
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      int v = cnt[t][q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WVN_WAVE);
      if ((threadIdx.x & (WVN_WAVE - 1)) == 0 && v != 0) atomicAdd(&ma_lds[nctr + t * 8 + q], (unsigned)v);
    }
  __syncthreads();
  for (int i = threadIdx.x; i < nctr; i += MA_THREADS) {
    const unsigned v = hist[i];
    if (v == 0u) continue;
    const int c = i & 1, t = (i >> 1) % NT, k = (i >> 1) / NT;
    atomicAdd((unsigned long long*)(d.state + (long long)(s * NT + t) * d.state_stride + 2 * k + c), (unsigned long long)v);
  }
  if (threadIdx.x < MA_TAIL) {
    const int t = threadIdx.x >> 3, q = threadIdx.x & 7;
    const unsigned v = ma_lds[nctr + threadIdx.x];
    if (t < NT && q < 7 && v != 0u)
      atomicAdd((unsigned long long*)(d.state + (long long)(s * NT + t) * d.state_stride + 2 * (T + 1) + q), (unsigned long long)v);
  }
}

// ---- block scans of 1024 threads (16 waves) --------------------------------------------------------------------------------
struct Sum { __device__ static long long op(long long a, long long b) { return a + b; } __device__ static long long id() { return 0; } };
struct Max { __device__ static long long op(long long a, long long b) { return a > b ? a : b; } __device__ static long long id() { return -1; } };

// inclusive scan over the threads of the block in thread order; *total = the value of the last thread.  sh: 17 words, reusable
// after the call (it ends with a barrier)
template <typename Op>
__device__ inline long long block_scan_incl(long long v, long long* sh, long long* total) {
  const int lane = threadIdx.x & (WVN_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < WVN_WAVE; o <<= 1) {
    const long long u = __shfl_up(v, o, WVN_WAVE);
    if (lane >= o) v = Op::op(v, u);
  }
  if (lane == WVN_WAVE - 1) sh[wave] = v;
  __syncthreads();
  long long before = Op::id();
  for (int w = 0; w < wave; ++w) before = Op::op(before, sh[w]);
  long long all = before;
  for (int w = wave; w < MC_THREADS / WVN_WAVE; ++w) all = Op::op(all, sh[w]);
  __syncthreads();
  *total = all;
  return Op::op(before, v);
}

extern __shared__ double mc_term[];

// one workgroup.  Thread i owns the bins of chunk (1023 - i): a scan in thread order is a suffix sum over the bins
__global__ __launch_bounds__(MC_THREADS) void metric_curve_kernel(const long long* __restrict__ state, const float* __restrict__ th, int T,
                                                                  double* fpr, double* tpr, double* __restrict__ thr,
                                                                  double* __restrict__ scal, long long* __restrict__ cnt) {
  __shared__ long long sh[MC_THREADS / WVN_WAVE + 1];
  const int per = (T + 1 + MC_THREADS - 1) / MC_THREADS;
  const int chunk = MC_THREADS - 1 - (int)threadIdx.x;
  const int lo = chunk * per < T + 1 ? chunk * per : T + 1;
  const int hi = lo + per < T + 1 ? lo + per : T + 1;
  long long lp = 0, ln = 0;
  for (int k = lo; k < hi; ++k) {
    ln += state[2 * k];
    lp += state[2 * k + 1];
  }
  long long P, N;
  const long long ip = block_scan_incl<Sum>(lp, sh, &P);
  const long long in = block_scan_incl<Sum>(ln, sh, &N);
  long long rp = ip - lp, rn = in - ln;   // the bins above this chunk
  const double dP = (double)P, dN = (double)N;
  for (int k = hi - 1; k >= lo; --k) {
    rn += state[2 * k];
    rp += state[2 * k + 1];   // = sum over bins >= k = tps[k - 1]
    if (k >= 1) {
      const int i = T - k;    // threshold t = k - 1 at flipped index T - 1 - t
      tpr[i] = P > 0 ? (double)rp / dP : 0.0;
      fpr[i] = N > 0 ? (double)rn / dN : 0.0;
      thr[i] = (double)th[k - 1];
    }
  }
  __syncthreads();
  for (int i = 1 + (int)threadIdx.x; i < T; i += MC_THREADS) {
    const double dx = fpr[i] - fpr[i - 1];
    const double sy = tpr[i] + tpr[i - 1];
    mc_term[i] = (dx * sy) * 0.5;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool degenerate = P == 0 || N == 0;
    double acc = 0.0;
    for (int i = 1; i < T; ++i) acc += mc_term[i];
    scal[0] = degenerate ? 0.0 : acc;
    const long long* cm = state + 2 * (T + 1);
    const long long all = cm[0] + cm[1] + cm[2] + cm[3];
    scal[1] = all > 0 ? (double)(cm[3] + cm[0]) / (double)all : 0.0;
    cnt[0] = P;
    cnt[1] = N;
    cnt[2] = degenerate ? 1 : 0;
  }
}

// one workgroup walks the entries in rounds of 1024 x MW_ITEMS.  With the exclusive prefixes Pp(e), Pn(e) of pos and neg and
// Hp(e), Hn(e) = those prefixes at the first entry of e's group,
//   U2 = sum_e neg_e (Hp(e) + Pp(e) + pos_e) + pos_e (Pn(e) - Hn(e))
// (adding entry e to its group raises neg_g (2 A + pos_g) by exactly that).  The prefixes never decrease, so "the prefix at the latest
// group head" is a running maximum: two sum scans and two max scans per round, the carries in registers.
__global__ __launch_bounds__(MC_THREADS) void metric_auroc_weighted_kernel(const float* __restrict__ score, const long long* __restrict__ pos,
                                                                           const long long* __restrict__ neg, long long E,
                                                                           double* __restrict__ scal, long long* __restrict__ cnt) {
  __shared__ long long sh[MC_THREADS / WVN_WAVE + 1];
  long long cp = 0, cn = 0, chp = 0, chn = 0;   // carries: sums so far, head prefixes so far
  unsigned long long u2 = 0;
  for (long long base = 0; base < E; base += (long long)MC_THREADS * MW_ITEMS) {
    const long long e0 = base + (long long)threadIdx.x * MW_ITEMS;
    float sc[MW_ITEMS];
    long long p[MW_ITEMS], n[MW_ITEMS];
    bool head[MW_ITEMS];
    long long lp = 0, ln = 0;
#pragma unroll
    for (int j = 0; j < MW_ITEMS; ++j) {
      const long long e = e0 + j;
      sc[j] = 0.f; p[j] = 0; n[j] = 0; head[j] = false;
      if (e < E) {
        sc[j] = score[e];
        const bool nan = sc[j] != sc[j];
        p[j] = nan ? 0 : pos[e];
        n[j] = nan ? 0 : neg[e];
        const float prev = j > 0 ? sc[j - 1] : (e > 0 ? score[e - 1] : 0.f);
        head[j] = e == 0 || !(sc[j] == prev);
      }
      lp += p[j];
      ln += n[j];
    }
    long long tp, tn, thp, thn;
    long long xp = cp + block_scan_incl<Sum>(lp, sh, &tp) - lp;   // exclusive prefix at this thread's first entry
    long long xn = cn + block_scan_incl<Sum>(ln, sh, &tn) - ln;
    long long mhp = -1, mhn = -1;
    {
      long long qp = xp, qn = xn;
#pragma unroll
      for (int j = 0; j < MW_ITEMS; ++j) {
        if (head[j]) { mhp = qp; mhn = qn; }
        qp += p[j];
        qn += n[j];
      }
    }
    // the head prefixes of the threads before this one (exclusive = inclusive scan of the value shifted by one thread)
    const long long ihp = block_scan_incl<Max>(mhp, sh, &thp);
    const long long ihn = block_scan_incl<Max>(mhn, sh, &thn);
    long long php = __shfl_up(ihp, 1, WVN_WAVE), phn = __shfl_up(ihn, 1, WVN_WAVE);
    __shared__ long long edge[2][MC_THREADS / WVN_WAVE];
    if ((threadIdx.x & (WVN_WAVE - 1)) == WVN_WAVE - 1) { edge[0][threadIdx.x >> 6] = ihp; edge[1][threadIdx.x >> 6] = ihn; }
    __syncthreads();
    if ((threadIdx.x & (WVN_WAVE - 1)) == 0) {
      const int w = threadIdx.x >> 6;
      php = w > 0 ? edge[0][w - 1] : -1;
      phn = w > 0 ? edge[1][w - 1] : -1;
    }
    __syncthreads();
    long long hp = php > chp ? php : chp, hn = phn > chn ? phn : chn;
#pragma unroll
    for (int j = 0; j < MW_ITEMS; ++j) {
      if (head[j]) { hp = xp; hn = xn; }
      u2 += (unsigned long long)n[j] * (unsigned long long)(hp + xp + p[j]) + (unsigned long long)p[j] * (unsigned long long)(xn - hn);
      xp += p[j];
      xn += n[j];
    }
    cp += tp;
    cn += tn;
    chp = thp > chp ? thp : chp;
    chn = thn > chn ? thn : chn;
  }
  long long total;
  block_scan_incl<Sum>((long long)u2, sh, &total);
  if (threadIdx.x == 0) {
    const bool degenerate = cp == 0 || cn == 0;
    scal[0] = degenerate ? 0.0 : (double)total / (double)(2 * cp * cn);
    cnt[0] = total;
    cnt[1] = cp;
    cnt[2] = cn;
    cnt[3] = degenerate ? 1 : 0;
  }
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int wvn_metric_accumulate(const wvn_metric_desc* d, void* stream) {
  if (!d) return WVN_ERR_ARG;
  if (d->n_scores < 1 || d->n_scores > 2 || d->n_targets < 1 || d->n_targets > 2) return WVN_ERR_ARG;
  if (d->B < 1 || d->H < 1 || d->W < 1) return WVN_ERR_ARG;
  const long long npix = (long long)d->B * d->H * d->W;
  if ((long long)d->H * d->W >= (1ll << 31) || npix >= (1ll << 31)) return WVN_ERR_ARG;
  if (d->T < 2 || d->T > WVN_METRIC_MAX_T) return WVN_ERR_ARG;
  if (!d->thresholds || misaligned(d->thresholds, 4) || !d->state || misaligned(d->state, 8)) return WVN_ERR_ARG;
  if (d->state_stride < 2ll * (d->T + 1) + WVN_METRIC_STATE_TAIL) return WVN_ERR_ARG;
  if (d->seg && ((d->seg_bytes != 4 && d->seg_bytes != 8) || misaligned(d->seg, (size_t)d->seg_bytes))) return WVN_ERR_ARG;
  if (d->seg_off && misaligned(d->seg_off, 8)) return WVN_ERR_ARG;
  if (d->seg_counts && (!d->seg || misaligned(d->seg_counts, 4))) return WVN_ERR_ARG;
  if (d->seg && !d->seg_off && (d->S < 1 || (long long)d->B * d->S >= (1ll << 27))) return WVN_ERR_ARG;
  int any_seg = 0;
  for (int i = 0; i < d->n_scores; ++i) {
    if (!d->score[i] || misaligned(d->score[i], 4)) return WVN_ERR_ARG;
    if (d->score_kind[i] != WVN_METRIC_DENSE && d->score_kind[i] != WVN_METRIC_PER_SEGMENT) return WVN_ERR_ARG;
    if (d->score_kind[i] == WVN_METRIC_PER_SEGMENT) {
      if (!d->seg || d->score_stride[i] < 1) return WVN_ERR_ARG;
      any_seg = 1;
    }
  }
  for (int j = 0; j < d->n_targets; ++j) {
    const int dt = d->target_dtype[j];
    if (dt != WVN_METRIC_U8 && dt != WVN_METRIC_I32 && dt != WVN_METRIC_F32) return WVN_ERR_ARG;
    if (!d->target[j] || (dt != WVN_METRIC_U8 && misaligned(d->target[j], 4))) return WVN_ERR_ARG;
    if (d->target_kind[j] != WVN_METRIC_DENSE && d->target_kind[j] != WVN_METRIC_PER_SEGMENT) return WVN_ERR_ARG;
    if (d->target_kind[j] == WVN_METRIC_PER_SEGMENT) {
      if (!d->seg || d->target_stride[j] < 1) return WVN_ERR_ARG;
      any_seg = 1;
    }
  }
  MaArgs a;
  a.d = *d;
  a.npix = (unsigned)npix;
  a.plane = (unsigned)((long long)d->H * d->W);
  a.any_seg = any_seg;
  int lds_words = (d->T + 1) * d->n_targets * 2 + MA_TAIL;
  if (d->seg_counts && lds_words < MA_SEG_WINDOW_WORDS) lds_words = MA_SEG_WINDOW_WORDS;
  const int lds = lds_words * (int)sizeof(unsigned);
  a.lds_words = lds_words;
  static LdsOptIn lds_opt_in;   // per device (common.h); T = 8192 with two targets: 131 KB
  if (const int rc = lds_opt_in(((WVN_METRIC_MAX_T + 1) * 4 + MA_TAIL) * (int)sizeof(unsigned), (const void*)metric_accumulate_kernel)) return rc;
  const long long groups = (npix + MA_PIX - 1) / MA_PIX;
  long long blocks = (groups + MA_THREADS - 1) / MA_THREADS;
  if (blocks > MA_MAX_BLOCKS) blocks = MA_MAX_BLOCKS;
  a.chunk = (unsigned)(((groups + blocks - 1) / blocks + MA_THREADS - 1) / MA_THREADS * MA_THREADS);
  hipLaunchKernelGGL(metric_accumulate_kernel, dim3((unsigned)blocks, d->n_scores + (d->seg_counts ? 1 : 0)), dim3(MA_THREADS), lds, (hipStream_t)stream, a);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

extern "C" int wvn_metric_curve(const long long* state, const float* thresholds, int T, double* fpr, double* tpr, double* thr, double* scal,
                                long long* cnt, void* stream) {
  if (T < 2 || T > WVN_METRIC_MAX_T) return WVN_ERR_ARG;
  if (!state || !thresholds || !fpr || !tpr || !thr || !scal || !cnt) return WVN_ERR_ARG;
  if (misaligned(state, 8) || misaligned(thresholds, 4) || misaligned(fpr, 8) || misaligned(tpr, 8) || misaligned(thr, 8) || misaligned(scal, 8) ||
      misaligned(cnt, 8))
    return WVN_ERR_ARG;
  static LdsOptIn lds_opt_in;   // the AUROC terms: 8 T bytes, 64 KB at T = 8192, beside the scan words
  if (const int rc = lds_opt_in(WVN_METRIC_MAX_T * (int)sizeof(double), (const void*)metric_curve_kernel)) return rc;
  hipLaunchKernelGGL(metric_curve_kernel, dim3(1), dim3(MC_THREADS), T * sizeof(double), (hipStream_t)stream, state, thresholds, T, fpr, tpr, thr,
                     scal, cnt);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

extern "C" int wvn_metric_auroc_weighted(const float* score, const long long* pos, const long long* neg, long long E, double* scal,
                                         long long* cnt, void* stream) {
  if (E < 1 || E > (1ll << 24)) return WVN_ERR_ARG;
  if (!score || !pos || !neg || !scal || !cnt) return WVN_ERR_ARG;
  if (misaligned(score, 4) || misaligned(pos, 8) || misaligned(neg, 8) || misaligned(scal, 8) || misaligned(cnt, 8)) return WVN_ERR_ARG;
  hipLaunchKernelGGL(metric_auroc_weighted_kernel, dim3(1), dim3(MC_THREADS), 0, (hipStream_t)stream, score, pos, neg, E, scal, cnt);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
