// Dense CRF with the permutohedral-lattice filter (Adams et al. 2010; the permutohedral.cpp that pydensecrf's DenseCRF2D runs):
// the unary, Potts update, symmetric normalisation, softmax and tie rule of csrc/dense_crf.hip, with every sum_j k_m(i, j) v_j
// replaced by the lattice's splat / blur / slice.  Reading, determinism and error budget: DESIGN.md "Permutohedral dense CRF".
//
// Per frame and lattice (Gaussian d = 2, bilateral d = 5), once per call:
//   lattice_build_kernel   one thread per pixel: features, elevation, rounding, rank, barycentric weights, d + 1 packed vertex keys
//   sort_*_kernel          stable LSD radix sort of (key, pixel (d+1) + r), 8-bit digits over the bits the key range needs
//   rows_*_kernel          unique keys -> table rows (1-based: row 0 is "no such lattice point"), each vertex's row, the CSR start of
//                          every lattice point's contributor list (pixel order), M
//   neighbour_kernel       blur neighbours by binary search in the sorted unique keys
// Filter (both lattices in one launch each): splat as a gather over the CSR lists in fixed order (aligned chunks of CH contributors
// that lie inside one point are summed by splat_part_kernel, added in chunk order by splat_sum_kernel), d + 1 blur passes, and the
// slice fused with the update epilogue (update_kernel).  No float atomics: results are bitwise reproducible and independent of the
// batch.  Compiled with -ffp-contract=off: the lattice construction is fp32, one operation at a time, as the source writes it.
#include <cmath>

#include "common.h"
#include "wvn_internal.h"
#include "../../include/wvn_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int ST = 256;            // threads of the sort / scan kernels
constexpr int SI = 8;              // elements per thread per sort tile
constexpr int TILE = ST * SI;      // sort tile
constexpr int CH = 64;             // splat chunk (contributors)
constexpr int GRID_CAP = 1024;     // workgroups per frame of the grid-stride kernels

struct Lattice {
  int d, E, NT, kbits;              // E = N (d + 1) vertices per frame, NT sort tiles, kbits key bits
  float sxy, srgb;                  // feature divisors
  float scale[5];                   // the diagonal of E (host: double, stored as float)
  int bias[5], sh[5], bits[5];      // packing: coordinate i -> ((key_i + bias_i) << sh_i), coordinate 0 most significant
  float alpha;                      // 1 / (1 + 2^-d)
  u64* key[2]; unsigned* val[2];    // [B][E] sort ping-pong (the sorted pair is key[0] / val[0] after an even number of passes)
  int fin;                          // which half holds the sorted pairs
  float* bary;                      // [B][E] barycentric weight of vertex pixel (d+1) + r
  int* vert;                        // [B][E] table row of vertex pixel (d+1) + r
  u64* ukey;                        // [B][E] unique keys, ascending
  int* start;                       // [B][E + 1] CSR start of each lattice point in the sorted order
  int2* nbr;                        // [B][d + 1][E] blur neighbour rows (n1, n2), 0 = absent
  int* M;                           // [B]
  float* tab[2];                    // [B][E + 1][KP] value tables (row 0: zeros, written by every splat and blur pass)
  float* part;                      // [B][E / CH][KP] chunk partial sums
  int* hist; int* tot; int* bsum;   // [B][256][NT], [B][256], [B][NT]
};

struct PermArgs {
  Lattice L[2];                     // 0: Gaussian (positions), 1: bilateral (positions and colour)
  const float* l1; long long s1b, s1c, s1p; int K1;
  const float* l2; long long s2b, s2c, s2p; int K2;
  const unsigned char* img;         // [B][N][3]
  int B, H, W, N, KT, KP;
  float w_pos, w_bi;
  float* negU; float* q;            // [B][N][KP]
  float* nrm[2];                    // [B][N]: n_g, n_b
  int* labels; float* probs; float* dbg;
};

// ------------------------------------------------------------------ lattice construction --------------------------------------------
__device__ inline bool pack_key(const Lattice& L, const int* k, u64& out) {
  u64 p = 0;
  for (int i = 0; i < L.d; ++i) {
    const long long c = (long long)k[i] + L.bias[i];
    if (c < 0 || c >= (1ll << L.bits[i])) return false;
    p |= (u64)c << L.sh[i];
  }
  out = p;
  return true;
}

__device__ inline int unpack_coord(const Lattice& L, u64 p, int i) {
  return (int)((p >> L.sh[i]) & ((1ull << L.bits[i]) - 1)) - L.bias[i];
}

// permutohedral.cpp Permutohedral::init for one feature vector, statement for statement
template <int D>
__global__ __launch_bounds__(256) void lattice_build_kernel(Lattice L, const unsigned char* __restrict__ img, int B, int H, int W) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = H * W;
  if (t >= (long long)B * N) return;
  const int b = (int)(t / N), p = (int)(t % N);
  float f[D];
  f[0] = (float)(p % W) / L.sxy;   // DenseCRF2D: feature(0) = i / sx, feature(1) = j / sy, colours im[..] / sr
  f[1] = (float)(p / W) / L.sxy;
  if constexpr (D == 5) {
    const unsigned char* c = img + ((size_t)b * N + p) * 3;
    f[2] = (float)c[0] / L.srgb;
    f[3] = (float)c[1] / L.srgb;
    f[4] = (float)c[2] / L.srgb;
  }
  float e[D + 1];
  float sm = 0.f;
#pragma unroll
  for (int j = D; j > 0; --j) {
    const float cf = f[j - 1] * L.scale[j - 1];
    e[j] = sm - (float)j * cf;
    sm += cf;
  }
  e[0] = sm;
  const float down_factor = 1.0f / (D + 1), up_factor = (float)(D + 1);
  float rem0[D + 1];
  int sum = 0;
#pragma unroll
  for (int i = 0; i <= D; ++i) {
    const float v = down_factor * e[i];
    const float up = ceilf(v) * up_factor, down = floorf(v) * up_factor;
    const int rd = (up - e[i] < e[i] - down) ? (int)(short)up : (int)(short)down;
    rem0[i] = (float)rd;
    sum = (int)((float)sum + (float)rd * down_factor);   // int sum; sum += rd2 * down_factor
  }
  int rank[D + 1];
#pragma unroll
  for (int i = 0; i <= D; ++i) rank[i] = 0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const float di = e[i] - rem0[i];
#pragma unroll
    for (int j = i + 1; j <= D; ++j) {
      if (di < e[j] - rem0[j]) rank[i]++;
      else rank[j]++;
    }
  }
#pragma unroll
  for (int i = 0; i <= D; ++i) {
    rank[i] += sum;
    if (rank[i] < 0) {
      rank[i] += D + 1;
      rem0[i] += (float)(D + 1);
    } else if (rank[i] > D) {
      rank[i] -= D + 1;
      rem0[i] -= (float)(D + 1);
    }
  }
  float bar[D + 2];
#pragma unroll
  for (int i = 0; i < D + 2; ++i) bar[i] = 0.f;
#pragma unroll
  for (int i = 0; i <= D; ++i) {
    const float v = (e[i] - rem0[i]) * down_factor;
    bar[D - rank[i]] += v;
    bar[D - rank[i] + 1] -= v;
  }
  bar[0] = (float)((double)bar[0] + (1.0 + (double)bar[D + 1]));   // barycentric[0] += 1.0 + barycentric[d+1]: a double expression
  const size_t o = (size_t)b * L.E + (size_t)p * (D + 1);
#pragma unroll
  for (int r = 0; r <= D; ++r) {
    int k[D];
#pragma unroll
    for (int i = 0; i < D; ++i) k[i] = (int)rem0[i] + (rank[i] <= D - r ? r : r - (D + 1));   // canonical[r][rank[i]]
    u64 pk = 0;
    pack_key(L, k, pk);   // in range by the host's bound (lattice_setup)
    L.key[0][o + r] = pk;
    L.val[0][o + r] = (unsigned)(p * (D + 1) + r);
    L.bary[o + r] = bar[r];
  }
}

// ------------------------------------------------------------------ sort and index ---------------------------------------------------
// exclusive scan over the 256 threads of a workgroup; *total receives the sum
__device__ inline int block_exclusive_scan(int x, int* total) {
  __shared__ int wsum[ST / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int s = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  if (lane == 63) wsum[w] = s;
  __syncthreads();
  int pre = 0, all = 0;
#pragma unroll
  for (int k = 0; k < ST / 64; ++k) {
    pre += k < w ? wsum[k] : 0;
    all += wsum[k];
  }
  __syncthreads();
  *total = all;
  return pre + s - x;
}

// per tile and digit counts: hist[b][digit][tile]
__global__ __launch_bounds__(ST) void sort_hist_kernel(Lattice L, int src, int shift) {
  __shared__ int h[256];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const u64* k = L.key[src] + (size_t)b * L.E;
  for (int it = 0; it < SI; ++it) {
    const int i = tile * TILE + it * ST + tid;
    if (i < L.E) atomicAdd(&h[(int)((k[i] >> shift) & 255)], 1);
  }
  __syncthreads();
  L.hist[((size_t)b * 256 + tid) * L.NT + tile] = h[tid];
}

// per digit: exclusive prefix over the tiles (in place) and the digit's total
__global__ __launch_bounds__(ST) void sort_digit_scan_kernel(Lattice L) {
  const int b = blockIdx.y, dg = blockIdx.x;
  int* h = L.hist + ((size_t)b * 256 + dg) * L.NT;
  int carry = 0;
  for (int s = 0; s < L.NT; s += ST) {
    const int i = s + threadIdx.x;
    const int x = i < L.NT ? h[i] : 0;
    int tot;
    const int ex = block_exclusive_scan(x, &tot);
    if (i < L.NT) h[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) L.tot[b * 256 + dg] = carry;
}

// stable scatter: within a tile, elements keep their order per digit (wave ballots give the rank among equal digits)
__global__ __launch_bounds__(ST) void sort_scatter_kernel(Lattice L, int src, int shift) {
  __shared__ int base[256], run[256], cnt[ST / 64][256];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  {
    int all;
    const int ex = block_exclusive_scan(L.tot[b * 256 + tid], &all);
    base[tid] = ex + L.hist[((size_t)b * 256 + tid) * L.NT + tile];
    run[tid] = 0;
  }
  const u64* kin = L.key[src] + (size_t)b * L.E;
  const unsigned* vin = L.val[src] + (size_t)b * L.E;
  u64* kout = L.key[src ^ 1] + (size_t)b * L.E;
  unsigned* vout = L.val[src ^ 1] + (size_t)b * L.E;
  const u64 lt = (1ull << lane) - 1;
  for (int it = 0; it < SI; ++it) {
#pragma unroll
    for (int k = 0; k < ST / 64; ++k) cnt[k][tid] = 0;
    __syncthreads();
    const int i = tile * TILE + it * ST + tid;
    const bool valid = i < L.E;
    const u64 key = valid ? kin[i] : 0;
    const unsigned v = valid ? vin[i] : 0;
    const int dg = (int)((key >> shift) & 255);
    u64 peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const u64 m = __ballot((dg >> bit) & 1);
      peers &= ((dg >> bit) & 1) ? m : ~m;
    }
    const int rank = __popcll(peers & lt);
    if (valid && rank == 0) cnt[w][dg] = __popcll(peers);
    __syncthreads();
    if (valid) {
      int pos = base[dg] + run[dg] + rank;
      for (int k = 0; k < w; ++k) pos += cnt[k][dg];
      kout[pos] = key;
      vout[pos] = v;
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int k = 0; k < ST / 64; ++k) add += cnt[k][tid];
    run[tid] += add;
  }
}

__device__ inline bool head_of(const u64* k, int i) { return i == 0 || k[i] != k[i - 1]; }

// unique keys per tile
__global__ __launch_bounds__(ST) void rows_count_kernel(Lattice L) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const u64* k = L.key[L.fin] + (size_t)b * L.E;
  int c = 0;
  for (int it = 0; it < SI; ++it) {
    const int i = tile * TILE + it * ST + threadIdx.x;
    c += (i < L.E && head_of(k, i)) ? 1 : 0;
  }
  int all;
  block_exclusive_scan(c, &all);
  if (threadIdx.x == 0) L.bsum[(size_t)b * L.NT + tile] = all;
}

__global__ __launch_bounds__(ST) void rows_tile_scan_kernel(Lattice L) {
  const int b = blockIdx.y;
  int* h = L.bsum + (size_t)b * L.NT;
  int carry = 0;
  for (int s = 0; s < L.NT; s += ST) {
    const int i = s + threadIdx.x;
    const int x = i < L.NT ? h[i] : 0;
    int tot;
    const int ex = block_exclusive_scan(x, &tot);
    if (i < L.NT) h[i] = carry + ex;
    carry += tot;
  }
}

// row of every sorted element (1 + the number of distinct keys before it), each vertex's row, the unique keys, CSR starts, M
__global__ __launch_bounds__(ST) void rows_emit_kernel(Lattice L) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const u64* k = L.key[L.fin] + (size_t)b * L.E;
  const unsigned* v = L.val[L.fin] + (size_t)b * L.E;
  int carry = L.bsum[(size_t)b * L.NT + tile];
  for (int it = 0; it < SI; ++it) {
    const int i = tile * TILE + it * ST + threadIdx.x;
    const int h = (i < L.E && head_of(k, i)) ? 1 : 0;
    int tot;
    const int ex = block_exclusive_scan(h, &tot);
    if (i < L.E) {
      const int row = carry + ex + h;   // 1-based
      L.vert[(size_t)b * L.E + v[i]] = row;
      if (h) {
        L.ukey[(size_t)b * L.E + row - 1] = k[i];
        L.start[(size_t)b * (L.E + 1) + row - 1] = i;
      }
      if (i == L.E - 1) {
        L.M[b] = row;
        L.start[(size_t)b * (L.E + 1) + row] = L.E;
      }
    }
    carry += tot;
  }
}

template <int D>
__device__ inline int find_row(const Lattice& L, const u64* uk, int M, const int* key) {
  u64 p;
  if (!pack_key(L, key, p)) return 0;
  int lo = 0, hi = M;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (uk[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return (lo < M && uk[lo] == p) ? lo + 1 : 0;
}

// blur neighbours of lattice point m along axis j (Permutohedral::init): n1 = key - 1 with coordinate j + d, n2 = key + 1 with
// coordinate j - d (axis d: all -1 / all +1)
template <int D>
__global__ __launch_bounds__(256) void neighbour_kernel(Lattice L) {
  const int b = blockIdx.y, M = L.M[b];
  const u64* uk = L.ukey + (size_t)b * L.E;
  for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
    int key[D];
#pragma unroll
    for (int i = 0; i < D; ++i) key[i] = unpack_coord(L, uk[m], i);
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      int n1[D], n2[D];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        n1[i] = key[i] - 1;
        n2[i] = key[i] + 1;
      }
      if (j < D) {
        n1[j] = key[j] + D;
        n2[j] = key[j] - D;
      }
      L.nbr[((size_t)b * (D + 1) + j) * L.E + m] = make_int2(find_row<D>(L, uk, M, n1), find_row<D>(L, uk, M, n2));
    }
  }
}

// ------------------------------------------------------------------ filter ------------------------------------------------------------
// value of contributor (sorted position i) in column c: barycentric weight times the input (ones, or n_m * Q)
template <int D>
__device__ inline float splat_term(const PermArgs& a, const Lattice& L, const float* nrm, int b, int i, int c, int ncol) {
  const unsigned v = L.val[L.fin][(size_t)b * L.E + i];
  const int pix = (int)(v / (D + 1));
  const float w = L.bary[(size_t)b * L.E + v];
  const float in = ncol == 1 ? 1.0f : nrm[(size_t)b * a.N + pix] * a.q[((size_t)b * a.N + pix) * a.KP + c];
  return w * in;
}

template <int D>
__device__ inline void splat_part(const PermArgs& a, const Lattice& L, const float* nrm, int ncol) {
  const int b = blockIdx.y, nch = L.E / CH;
  const u64* k = L.key[L.fin] + (size_t)b * L.E;
  const long long items = (long long)nch * ncol;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (long long)gridDim.x * blockDim.x) {
    const int ch = (int)(t / ncol), c = (int)(t % ncol);
    const int s = ch * CH;
    if (k[s] != k[s + CH - 1]) continue;   // not inside one lattice point: its points sum these contributors directly
    float acc = 0.f;
    for (int i = s; i < s + CH; ++i) acc += splat_term<D>(a, L, nrm, b, i, c, ncol);
    L.part[((size_t)b * nch + ch) * ncol + c] = acc;
  }
}

// point m: contributors [s, e) in pixel order; the aligned chunks [c0, c1) inside it come from splat_part, in chunk order
template <int D>
__device__ inline void splat_sum(const PermArgs& a, const Lattice& L, const float* nrm, int ncol) {
  const int b = blockIdx.y, M = L.M[b], nch = L.E / CH;
  const int* st = L.start + (size_t)b * (L.E + 1);
  float* out = L.tab[0] + (size_t)b * (L.E + 1) * a.KP;
  const long long items = (long long)M * ncol;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(t / ncol), c = (int)(t % ncol);
    const int s = st[m], e = st[m + 1];
    const int c0 = (s + CH - 1) / CH, c1 = e / CH;
    float acc = 0.f;
    if (c0 < c1) {
      for (int i = s; i < c0 * CH; ++i) acc += splat_term<D>(a, L, nrm, b, i, c, ncol);
      for (int ch = c0; ch < c1; ++ch) acc += L.part[((size_t)b * nch + ch) * ncol + c];
      for (int i = c1 * CH; i < e; ++i) acc += splat_term<D>(a, L, nrm, b, i, c, ncol);
    } else {
      for (int i = s; i < e; ++i) acc += splat_term<D>(a, L, nrm, b, i, c, ncol);
    }
    out[(size_t)(m + 1) * ncol + c] = acc;
    if (m == 0) out[c] = 0.f;   // row 0 at this stride ("no such lattice point")
  }
}

// blockIdx.z = lattice; ncol == 1: the normaliser pass (unit values)
__global__ __launch_bounds__(256) void splat_part_kernel(PermArgs a, int ncol) {
  if (blockIdx.z == 0) splat_part<2>(a, a.L[0], a.nrm[0], ncol);
  else splat_part<5>(a, a.L[1], a.nrm[1], ncol);
}

__global__ __launch_bounds__(256) void splat_sum_kernel(PermArgs a, int ncol) {
  if (blockIdx.z == 0) splat_sum<2>(a, a.L[0], a.nrm[0], ncol);
  else splat_sum<5>(a, a.L[1], a.nrm[1], ncol);
}

// blur along axis j: new = old + 0.5 (v[n1] + v[n2]), tab[j & 1] -> tab[(j + 1) & 1]
template <int D>
__device__ inline void blur(const PermArgs& a, const Lattice& L, int j, int ncol) {
  if (j > D) return;
  const int b = blockIdx.y, M = L.M[b];
  const float* in = L.tab[j & 1] + (size_t)b * (L.E + 1) * a.KP;
  float* out = L.tab[(j + 1) & 1] + (size_t)b * (L.E + 1) * a.KP;
  const int2* nb = L.nbr + ((size_t)b * (D + 1) + j) * L.E;
  const long long items = (long long)M * ncol;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(t / ncol), c = (int)(t % ncol);
    const int2 n = nb[m];
    out[(size_t)(m + 1) * ncol + c] = in[(size_t)(m + 1) * ncol + c] + 0.5f * (in[(size_t)n.x * ncol + c] + in[(size_t)n.y * ncol + c]);
    if (m == 0) out[c] = 0.f;
  }
}

// gridDim.z == 2: both lattices; 1: the bilateral lattice alone (axes 3..5)
__global__ __launch_bounds__(256) void blur_kernel(PermArgs a, int j, int ncol) {
  if (gridDim.z == 2 && blockIdx.z == 0) blur<2>(a, a.L[0], j, ncol);
  else blur<5>(a, a.L[1], j, ncol);
}

// slice of pixel p in column c: sum_r (b_r v[vertex_r]) alpha, r = 0..d in order
template <int D>
__device__ inline float slice(const PermArgs& a, const Lattice& L, int b, int p, int c, int ncol) {
  const float* tab = L.tab[(D + 1) & 1] + (size_t)b * (L.E + 1) * a.KP;
  const size_t o = (size_t)b * L.E + (size_t)p * (D + 1);
  float s = 0.f;
#pragma unroll
  for (int r = 0; r <= D; ++r) s += (L.bary[o + r] * tab[(size_t)L.vert[o + r] * ncol + c]) * L.alpha;
  return s;
}

// normalisers n_m = 1 / sqrt(filter_m(1) + 1e-20) (a double expression in the source), the unary -U and Q^0 (as csrc/dense_crf.hip)
__global__ __launch_bounds__(256) void perm_prep_kernel(PermArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.B * a.N) return;
  const int b = (int)(i / a.N), p = (int)(i % a.N);
  a.nrm[0][i] = (float)(1.0 / sqrt((double)slice<2>(a, a.L[0], b, p, 0, 1) + 1e-20));
  a.nrm[1][i] = (float)(1.0 / sqrt((double)slice<5>(a, a.L[1], b, p, 0, 1) + 1e-20));
  const size_t row = (size_t)i * a.KP;
  for (int grp = 0; grp < 2; ++grp) {
    const float* Lg = grp ? a.l2 : a.l1;
    const int K = grp ? a.K2 : a.K1, off = grp ? a.K1 : 0;
    if (K == 0) continue;
    const long long sb = grp ? a.s2b : a.s1b, sc = grp ? a.s2c : a.s1c, sp = grp ? a.s2p : a.s1p;
    const float* l = Lg + b * sb + p * sp;
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) m = fmaxf(m, l[k * sc]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(l[k * sc] - m);
    float m2 = -INFINITY;
    for (int k = 0; k < K; ++k) {   // -U = log(clip(softmax(L), 1e-5, 1))
      const float u = logf(fminf(fmaxf(expf(l[k * sc] - m) / s, 1e-5f), 1.0f));
      a.negU[row + off + k] = u;
      m2 = fmaxf(m2, u);
    }
    float s2 = 0.f;
    for (int k = 0; k < K; ++k) s2 += expf(a.negU[row + off + k] - m2);
    for (int k = 0; k < K; ++k) a.q[row + off + k] = expf(a.negU[row + off + k] - m2) / s2;   // Q^0 = softmax(-U)
  }
  for (int c = a.KT; c < a.KP; ++c) {
    a.negU[row + c] = 0.f;
    a.q[row + c] = 0.f;
  }
}

// KP lanes per pixel (lane = value column): slice both lattices, -U + pos_w msg_g + bi_w msg_b, softmax per CRF group, Q in place
__global__ __launch_bounds__(256) void update_kernel(PermArgs a, int last) {
  const int b = blockIdx.y, KP = a.KP;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = t / KP, c = t % KP;
  const bool live = p < a.N;
  const int pc = live ? p : a.N - 1;
  const size_t pix = (size_t)b * a.N + pc;
  const float ng = a.nrm[0][pix], nb = a.nrm[1][pix];
  const float mg = ng * slice<2>(a, a.L[0], b, pc, c, KP);
  const float mb = nb * slice<5>(a, a.L[1], b, pc, c, KP);
  float lg = a.negU[pix * KP + c] + a.w_pos * mg;   // pydensecrf: tmp1 = -U; tmp1 -= -w_g msg_g; tmp1 -= -w_b msg_b
  lg = lg + a.w_bi * mb;
  const bool valid = c < a.KT;
  const int grp = c >= a.K1;
  float gmax[2], gsum[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float v = valid && grp == s ? lg : -INFINITY;
    for (int o = KP / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    gmax[s] = v;
  }
  const float ev = valid ? expf(lg - gmax[grp]) : 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float v = grp == s ? ev : 0.f;
    for (int o = KP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    gsum[s] = v;
  }
  const float qv = valid ? ev / gsum[grp] : 0.f;
  if (live) a.q[pix * KP + c] = qv;
  if (!last) return;
  // first maximum per group
  int ng_ = a.K2 > 0 ? 2 : 1;
  int arg[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float bv = valid && grp == s ? qv : -INFINITY;
    int bi = valid && grp == s ? c : 0x7fffffff;
    for (int o = KP / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    arg[s] = bi;
  }
  if (!live) return;
  if (valid) {
    if (a.probs) a.probs[((size_t)b * a.KT + c) * a.N + p] = qv;
    if (a.dbg) {
      a.dbg[((size_t)b * (2 * KP + 2) + c) * a.N + p] = mb;
      a.dbg[((size_t)b * (2 * KP + 2) + KP + c) * a.N + p] = mg;
    }
  }
  if (c == 0) {
    if (a.labels)
      for (int s = 0; s < ng_; ++s) a.labels[((size_t)b * ng_ + s) * a.N + p] = arg[s] - (s ? a.K1 : 0);
    if (a.dbg) {
      a.dbg[((size_t)b * (2 * KP + 2) + 2 * KP) * a.N + p] = nb;
      a.dbg[((size_t)b * (2 * KP + 2) + 2 * KP + 1) * a.N + p] = ng;
    }
  }
}

// debug: the lattice structure of one lattice (keys unpacked, rows, weights, neighbours)
template <int D>
__global__ __launch_bounds__(256) void lattice_dump_kernel(Lattice L, int N, int* M, int* keys, float* bary, int* vert, int* nbr) {
  const int b = blockIdx.y;
  const int Mb = L.M[b];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.E; i += gridDim.x * blockDim.x) {
    const size_t o = (size_t)b * L.E + i;
    if (i == 0) M[b] = Mb;
    bary[o] = L.bary[o];
    vert[o] = L.vert[o];
#pragma unroll
    for (int k = 0; k < D; ++k) keys[o * D + k] = i < Mb ? unpack_coord(L, L.ukey[o], k) : 0;
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      const int2 n = i < Mb ? L.nbr[((size_t)b * (D + 1) + j) * L.E + i] : make_int2(0, 0);
      nbr[(((size_t)b * (D + 1) + j) * L.E + i) * 2] = n.x;
      nbr[(((size_t)b * (D + 1) + j) * L.E + i) * 2 + 1] = n.y;
    }
  }
}

// ------------------------------------------------------------------ host --------------------------------------------------------------
// scale factors and the key packing for features f_i in [0, fmax_i]: the host bound of every vertex coordinate (elevated range,
// rounding by <= (d+1)/2, the rank wrap by d+1, the canonical offset in [-d, d], slack) must fit pydensecrf's 16-bit keys and, packed,
// 64 bits.
bool lattice_setup(int d, int H, int W, float sxy, float srgb, Lattice& L) {
  if (!(sxy > 0.f) || !std::isfinite(sxy) || (d == 5 && (!(srgb > 0.f) || !std::isfinite(srgb)))) return false;
  L.d = d;
  L.sxy = sxy;
  L.srgb = srgb;
  const float inv_std_dev = (float)(std::sqrt(2.0 / 3.0) * (d + 1));
  double fmax[5] = {(double)((float)(W - 1) / sxy), (double)((float)(H - 1) / sxy), 0, 0, 0};
  for (int i = 2; i < d; ++i) fmax[i] = (double)(255.0f / srgb);
  double C[6] = {0, 0, 0, 0, 0, 0};   // C[j]: bound of cf_j = f[j-1] scale[j-1]
  for (int i = 0; i < d; ++i) {
    L.scale[i] = (float)(1.0 / std::sqrt((double)((i + 2) * (i + 1))) * inv_std_dev);
    C[i + 1] = fmax[i] * L.scale[i] * (1 + 1e-6);
  }
  const double slack = 3.0 * (d + 1) + 2;
  int total = 0;
  for (int j = 0; j < d; ++j) {
    double hi = 0;
    for (int k = j + 1; k <= d; ++k) hi += C[k];
    const double lo = j == 0 ? 0.0 : -(double)j * C[j];
    const double clo = std::floor(lo - slack), chi = std::ceil(hi + slack);
    if (clo < -32768.0 || chi > 32767.0) return false;
    const long long span = (long long)(chi - clo) + 1;
    int bits = 1;
    while ((1ll << bits) < span) ++bits;
    L.bias[j] = -(int)clo;
    L.bits[j] = bits;
    total += bits;
  }
  if (total > 64) return false;
  int sh = 0;
  for (int j = d - 1; j >= 0; --j) {
    L.sh[j] = sh;
    sh += L.bits[j];
  }
  L.kbits = total;
  L.alpha = 1.0f / (1 + powf(2.f, (float)-d));
  return true;
}

struct PermLayout {
  size_t negU, q, ng, nb, total;
  struct Lat { size_t key0, key1, val0, val1, bary, vert, ukey, start, nbr, M, tab0, tab1, part, hist, tot, bsum; } L[2];
};

PermLayout perm_layout(int B, int N, int KT) {
  const size_t KP = KT <= 32 ? 32 : 64;
  PermLayout l;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
  l.negU = take((size_t)B * N * KP * 4);
  l.q = take((size_t)B * N * KP * 4);
  l.ng = take((size_t)B * N * 4);
  l.nb = take((size_t)B * N * 4);
  for (int li = 0; li < 2; ++li) {
    const int d = li ? 5 : 2;
    const size_t E = (size_t)N * (d + 1), NT = (E + TILE - 1) / TILE;
    PermLayout::Lat& t = l.L[li];
    t.key0 = take(B * E * 8); t.key1 = take(B * E * 8);
    t.val0 = take(B * E * 4); t.val1 = take(B * E * 4);
    t.bary = take(B * E * 4); t.vert = take(B * E * 4);
    t.ukey = take(B * E * 8); t.start = take(B * (E + 1) * 4);
    t.nbr = take(B * (d + 1) * E * 8); t.M = take((size_t)B * 4);
    t.tab0 = take(B * (E + 1) * KP * 4); t.tab1 = take(B * (E + 1) * KP * 4);
    t.part = take(B * (E / CH) * KP * 4);
    t.hist = take(B * 256 * NT * 4); t.tot = take((size_t)B * 256 * 4); t.bsum = take(B * NT * 4);
  }
  l.total = o;
  return l;
}

bool perm_shape_ok(int B, int H, int W, int K1, int K2) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 2048 && W <= 2048 && K1 >= 1 && K2 >= 0 && K1 + K2 <= 64;
}

void bind_lattice(Lattice& L, const PermLayout::Lat& t, unsigned char* ws, int N) {
  L.E = N * (L.d + 1);
  L.NT = (L.E + TILE - 1) / TILE;
  L.key[0] = (u64*)(ws + t.key0); L.key[1] = (u64*)(ws + t.key1);
  L.val[0] = (unsigned*)(ws + t.val0); L.val[1] = (unsigned*)(ws + t.val1);
  L.bary = (float*)(ws + t.bary); L.vert = (int*)(ws + t.vert);
  L.ukey = (u64*)(ws + t.ukey); L.start = (int*)(ws + t.start);
  L.nbr = (int2*)(ws + t.nbr); L.M = (int*)(ws + t.M);
  L.tab[0] = (float*)(ws + t.tab0); L.tab[1] = (float*)(ws + t.tab1);
  L.part = (float*)(ws + t.part);
  L.hist = (int*)(ws + t.hist); L.tot = (int*)(ws + t.tot); L.bsum = (int*)(ws + t.bsum);
  L.fin = 0;
}

unsigned stride_grid(long long items) { return (unsigned)std::min<long long>((items + 255) / 256, GRID_CAP); }

// lattice build, sort, rows, neighbours of one lattice for every frame
int build_lattice(Lattice& L, const unsigned char* img, int B, int H, int W, hipStream_t st) {
  const int N = H * W;
  const unsigned gp = (unsigned)(((long long)B * N + 255) / 256);
  if (L.d == 2) hipLaunchKernelGGL(lattice_build_kernel<2>, dim3(gp), dim3(256), 0, st, L, img, B, H, W);
  else hipLaunchKernelGGL(lattice_build_kernel<5>, dim3(gp), dim3(256), 0, st, L, img, B, H, W);
  WVN_LAUNCH_CHECK();
  int src = 0;
  for (int shift = 0; shift < L.kbits; shift += 8, src ^= 1) {
    hipLaunchKernelGGL(sort_hist_kernel, dim3(L.NT, B), dim3(ST), 0, st, L, src, shift);
    WVN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sort_digit_scan_kernel, dim3(256, B), dim3(ST), 0, st, L);
    WVN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(L.NT, B), dim3(ST), 0, st, L, src, shift);
    WVN_LAUNCH_CHECK();
  }
  L.fin = src;
  hipLaunchKernelGGL(rows_count_kernel, dim3(L.NT, B), dim3(ST), 0, st, L);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(rows_tile_scan_kernel, dim3(1, B), dim3(ST), 0, st, L);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(rows_emit_kernel, dim3(L.NT, B), dim3(ST), 0, st, L);
  WVN_LAUNCH_CHECK();
  if (L.d == 2) hipLaunchKernelGGL(neighbour_kernel<2>, dim3(stride_grid(L.E), B), dim3(256), 0, st, L);
  else hipLaunchKernelGGL(neighbour_kernel<5>, dim3(stride_grid(L.E), B), dim3(256), 0, st, L);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

// one filter of both lattices with ncol value columns: result in tab[(d + 1) & 1] of each lattice
int filter_both(const PermArgs& a, int ncol, hipStream_t st) {
  const long long items = (long long)a.L[1].E * ncol;
  const dim3 grid(stride_grid(items), a.B, 2);
  hipLaunchKernelGGL(splat_part_kernel, grid, dim3(256), 0, st, a, ncol);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(splat_sum_kernel, grid, dim3(256), 0, st, a, ncol);
  WVN_LAUNCH_CHECK();
  for (int j = 0; j <= 5; ++j) {
    hipLaunchKernelGGL(blur_kernel, dim3(grid.x, a.B, j <= 2 ? 2 : 1), dim3(256), 0, st, a, j, ncol);
    WVN_LAUNCH_CHECK();
  }
  return WVN_OK;
}

}  // namespace

extern "C" {

size_t wvn_dense_crf_permutohedral_workspace_bytes(int B, int H, int W, int K) {
  if (!perm_shape_ok(B, H, W, K, 0)) return 0;
  return perm_layout(B, H * W, K).total;
}

int wvn_dense_crf_permutohedral(const float* logits1, int K1, long long s1b, long long s1c, long long s1p, const float* logits2, int K2,
                                long long s2b, long long s2c, long long s2p, const unsigned char* image, int B, int H, int W, int iterations,
                                float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, int* labels, int* nseg_last,
                                float* probs, float* debug, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logits1 || !image || !workspace || !perm_shape_ok(B, H, W, K1, K2) || (K2 > 0) != (logits2 != nullptr)) return WVN_ERR_ARG;
  if (nseg_last && !labels) return WVN_ERR_ARG;
  if (!labels && !probs && !debug) return WVN_ERR_ARG;
  if (iterations < 1 || iterations > 1000) return WVN_ERR_ARG;
  if (!std::isfinite(pos_w) || !std::isfinite(bi_w)) return WVN_ERR_ARG;
  PermArgs a;
  if (!lattice_setup(2, H, W, pos_xy_std, 0.f, a.L[0]) || !lattice_setup(5, H, W, bi_xy_std, bi_rgb_std, a.L[1])) return WVN_ERR_ARG;
  const int N = H * W, KT = K1 + K2;
  const PermLayout l = perm_layout(B, N, KT);
  if (workspace_bytes < l.total) return WVN_ERR_WORKSPACE;
  unsigned char* ws = (unsigned char*)workspace;
  a.l1 = logits1; a.s1b = s1b; a.s1c = s1c; a.s1p = s1p; a.K1 = K1;
  a.l2 = logits2; a.s2b = s2b; a.s2c = s2c; a.s2p = s2p; a.K2 = K2;
  a.img = image;
  a.B = B; a.H = H; a.W = W; a.N = N; a.KT = KT; a.KP = KT <= 32 ? 32 : 64;
  a.w_pos = pos_w; a.w_bi = bi_w;
  a.negU = (float*)(ws + l.negU); a.q = (float*)(ws + l.q);
  a.nrm[0] = (float*)(ws + l.ng); a.nrm[1] = (float*)(ws + l.nb);
  a.labels = labels; a.probs = probs; a.dbg = debug;
  hipStream_t st = (hipStream_t)stream;
  for (int li = 0; li < 2; ++li) {
    bind_lattice(a.L[li], l.L[li], ws, N);
    const int rc = build_lattice(a.L[li], image, B, H, W, st);
    if (rc) return rc;
  }
  int rc = filter_both(a, 1, st);   // the normalisers
  if (rc) return rc;
  hipLaunchKernelGGL(perm_prep_kernel, dim3((unsigned)(((long long)B * N + 255) / 256)), dim3(256), 0, st, a);
  WVN_LAUNCH_CHECK();
  const dim3 ugrid((unsigned)(((long long)N * a.KP + 255) / 256), B);
  for (int t = 1; t <= iterations; ++t) {
    rc = filter_both(a, a.KP, st);
    if (rc) return rc;
    hipLaunchKernelGGL(update_kernel, ugrid, dim3(256), 0, st, a, (int)(t == iterations));
    WVN_LAUNCH_CHECK();
  }
  if (nseg_last) {   // the k-means relabel rule on the last group, as the exact CRF
    const int ng = K2 > 0 ? 2 : 1;
    for (int b = 0; b < B; ++b) {
      rc = wvn_km_relabel_launch(labels + ((size_t)b * ng + ng - 1) * N, nseg_last + b, 1, N, ng == 2 ? K2 : K1, 1, st);
      if (rc) return rc;
    }
  }
  return WVN_OK;
}

int wvn_debug_permutohedral_lattice(const unsigned char* image, int B, int H, int W, int bilateral, float xy_std, float rgb_std, int* M,
                                    int* keys, float* bary, int* vert, int* nbr, void* workspace, size_t workspace_bytes, void* stream) {
  if (!image || !M || !keys || !bary || !vert || !nbr || !workspace || !perm_shape_ok(B, H, W, 1, 0)) return WVN_ERR_ARG;
  Lattice L;
  if (!lattice_setup(bilateral ? 5 : 2, H, W, xy_std, rgb_std, L)) return WVN_ERR_ARG;
  const PermLayout l = perm_layout(B, H * W, 1);
  if (workspace_bytes < l.total) return WVN_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  bind_lattice(L, l.L[bilateral ? 1 : 0], (unsigned char*)workspace, H * W);
  const int rc = build_lattice(L, image, B, H, W, st);
  if (rc) return rc;
  if (bilateral) hipLaunchKernelGGL(lattice_dump_kernel<5>, dim3(stride_grid(L.E), B), dim3(256), 0, st, L, H * W, M, keys, bary, vert, nbr);
  else hipLaunchKernelGGL(lattice_dump_kernel<2>, dim3(stride_grid(L.E), B), dim3(256), 0, st, L, H * W, M, keys, bary, vert, nbr);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

}  // extern "C"
