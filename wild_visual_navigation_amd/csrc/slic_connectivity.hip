// Connectivity enforcement for label maps (the post-processing step of SLIC, Achanta et al. 2012; fast_slic's Slic(...) does it by
// default): 4-connected fragments smaller than min_size are handed to a neighbouring superpixel.  Opt-in post-pass of ops.slic
// (enforce_connectivity=True); any int32 label map with ids in [0, K) is accepted.  PARITY WITH fast_slic's OWN POST-PASS IS UNPINNED
// (the package is absent, as for the SLIC itself): this is an ORDER-INDEPENDENT form of Achanta's sequential scan, held bit for bit to
// the plain statement in tests/slic_connectivity_ref.py:
//   1. a component is a maximal 4-connected set of equal-label pixels; 2. it is anchored when its size is >= min_size (no anchored
//   component: the map is returned as it is); 3. a round reads the state at its start: every waiting component that has a pair
//   (p inside, q a 4-neighbour of p in the frame, q anchored) counts such pairs per current label of q and takes the label with the
//   highest count (lowest id on a tie); it is anchored from the next round on; 4. rounds repeat until nothing waits.
// Two waiting components of one label never touch, so ONE component labelling of the input serves all rounds: the state is per
// component (current label, the round in which it was anchored), keyed by the component's smallest linear pixel index.
//
// Launch sequence for [B][H][W] maps (no host read anywhere; everything integer, ordinary vector stores and vector atomics):
//   cc_tile   union-find of a TH x TW tile in LDS -> parent[] holds the tile-local root (as a frame index)
//   cc_merge  unions across tile borders with atomicMin on parent[]
//   cc_flatten  parent[p] <- root (smallest index of the component), size[root] += 1
//   classify  roots: anchored (stamp 0) or waiting (stamp WAITING, appended to the image's list, a slice of plist reserved)
//   scatter   pixels of waiting components -> their slice of plist (the order inside a slice is arbitrary and never matters)
//   round x PAR_ROUNDS   one wave per waiting component: votes over its pixels' neighbours, arg-max, new label + stamp = round
//   tail      one workgroup per image runs further rounds until the image's counter of waiting components is zero (a no-op for the
//             maps SLIC produces: 3 - 7 rounds measured; chains longer than PAR_ROUNDS finish here, slower but complete)
//   relabel   out[p] = label of p's component
// "anchored at the start of round r" is stamp < r: a component absorbed in round r carries stamp r and is invisible to that round.
#include "../../include/wvn_hip.h"

#include "common.h"
#include "wvn_internal.h"

namespace {

constexpr int TW = WVN_SLIC_CC_TILE_W, TH = WVN_SLIC_CC_TILE_H;   // 32 x 8 = one pixel per thread of a 256-thread workgroup
constexpr int WAITING = 0x7fffffff;
constexpr int PAR_ROUNDS = WVN_SLIC_CC_PAR_ROUNDS;
constexpr int TAIL_THREADS = 1024;
// per-image counters at the head of the scratch buffer
enum { C_REMAINING = 0, C_NWAIT = 1, C_NANCH = 2, C_CURSOR = 3, C_STRIDE = 4 };

__device__ inline int ld_relaxed(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_relaxed(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Both find loops end: a parent is never larger than its child (par[i] <= i holds at initialisation and atomicMin only lowers an
// entry), and the walk stops at the first i with par[i] == i, so i strictly decreases and is bounded below by 0.
__device__ inline int find_lds(volatile int* par, int i) {
  int p;
  while ((p = par[i]) != i) i = p;
  return i;
}
__device__ inline int find_glb(const int* par, int i) {
  int p;
  while ((p = ld_relaxed(par + i)) != i) i = p;
  return i;
}
// Lock-free union (link the larger root under the smaller).  Ends: every failed atomicMin returns a value strictly below the root it
// was tried on (someone else lowered it), so max(a, b) strictly decreases from one iteration to the next.
__device__ inline void union_lds(int* par, int a, int b) {
  while (true) {
    a = find_lds(par, a); b = find_lds(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
}
__device__ inline void union_glb(int* par, int a, int b) {
  while (true) {
    a = find_glb(par, a); b = find_glb(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(TW * TH) void cc_tile_kernel(const int* __restrict__ labels, int* __restrict__ parent, int H, int W) {
  __shared__ int lab[TW * TH];
  __shared__ int par[TW * TH];
  const int t = threadIdx.x, lx = t % TW, ly = t / TW;
  const int x = blockIdx.x * TW + lx, y = blockIdx.y * TH + ly;
  const size_t img = (size_t)blockIdx.z * H * W;
  const bool in = x < W && y < H;
  const int l = in ? labels[img + (size_t)y * W + x] : 0;
  lab[t] = l; par[t] = t;
  __syncthreads();
  if (in) {   // (the left and upper neighbours of an in-frame pixel of this tile are in the frame)
    if (lx > 0 && lab[t - 1] == l) union_lds(par, t, t - 1);
    if (ly > 0 && lab[t - TW] == l) union_lds(par, t, t - TW);
  }
  __syncthreads();
  if (in) {
    // row-major order inside the tile agrees with row-major order in the frame: the tile-local root is the smallest frame index too
    const int r = find_lds(par, t);
    parent[img + (size_t)y * W + x] = (blockIdx.y * TH + r / TW) * W + blockIdx.x * TW + r % TW;
  }
}

__global__ __launch_bounds__(256) void cc_merge_kernel(const int* __restrict__ labels, int* __restrict__ parent, int H, int W) {
  const int npix = H * W;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const int y = p / W, x = p - y * W;
  const bool left = x > 0 && x % TW == 0, up = y > 0 && y % TH == 0;
  if (!left && !up) return;
  const size_t img = (size_t)blockIdx.y * npix;
  const int l = labels[img + p];
  if (left && labels[img + p - 1] == l) union_glb(parent + img, p, p - 1);
  if (up && labels[img + p - W] == l) union_glb(parent + img, p, p - W);
}

// parent[p] <- root.  In place while other lanes still walk: any value an entry holds during this kernel is an ancestor of p
// (its old parent or the root), so every walk still ends at the root.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, int* __restrict__ size, int npix) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const size_t img = (size_t)blockIdx.y * npix;
  const int r = find_glb(parent + img, p);
  st_relaxed(parent + img + p, r);
  atomicAdd(size + img + r, 1);
}

__global__ __launch_bounds__(256) void classify_kernel(const int* __restrict__ labels, const int* __restrict__ root,
                                                       const int* __restrict__ size, int* __restrict__ stamp, int* __restrict__ ulabel,
                                                       int* __restrict__ slice, int* __restrict__ wlist, int* __restrict__ cnt, int npix,
                                                       int min_size) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const size_t img = (size_t)blockIdx.y * npix;
  if (root[img + p] != p) return;
  int* c = cnt + blockIdx.y * C_STRIDE;
  ulabel[img + p] = labels[img + p];
  const int n = size[img + p];
  if (n >= min_size) {
    stamp[img + p] = 0;
    atomicAdd(c + C_NANCH, 1);
  } else {
    stamp[img + p] = WAITING;
    wlist[img + atomicAdd(c + C_NWAIT, 1)] = p;        // at most one entry per pixel: < npix
    slice[img + p] = atomicAdd(c + C_CURSOR, n);       // slices are disjoint and sum to <= npix
    atomicAdd(c + C_REMAINING, 1);
  }
}

// after this kernel slice[root] is the END of the component's slice of plist (the start is slice[root] - size[root])
__global__ __launch_bounds__(256) void scatter_kernel(const int* __restrict__ root, const int* __restrict__ stamp, int* __restrict__ slice,
                                                      int* __restrict__ plist, int npix) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const size_t img = (size_t)blockIdx.y * npix;
  const int r = root[img + p];
  if (stamp[img + r] != WAITING) return;
  plist[img + atomicAdd(slice + img + r, 1)] = p;
}

struct Maps { const int* root; const int* size; const int* slice; const int* plist; int* stamp; int* ulabel; };

// One wave decides one waiting component c in round r (all pointers are the image's own).  The votes are never stored: pass i counts
// the pairs whose label is the i-th smallest neighbouring label and finds the next larger one, so the candidates arrive in
// ascending order and "strictly more pairs" keeps the lowest id on a tie.  The loop ends: `target` strictly increases and takes only
// labels that occur among the (finitely many) pairs.
__device__ inline void decide_component(const Maps& m, int* cnt, int c, int r, int H, int W, int lane) {
  if (ld_relaxed(m.stamp + c) != WAITING) return;   // absorbed in an earlier round (wave-uniform: one c per wave)
  const int n = m.size[c], beg = m.slice[c] - n;
  const long long none = 0x7fffffffffffffffll;
  long long target = -none;
  int best = 0, best_count = 0;
  while (true) {
    int count = 0;
    long long next = none;
    for (int i = lane; i < n; i += WVN_WAVE) {
      const int p = m.plist[beg + i];
      const int y = p / W, x = p - y * W;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int qx = x + (d == 0 ? -1 : d == 1 ? 1 : 0), qy = y + (d == 2 ? -1 : d == 3 ? 1 : 0);
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const int rq = m.root[qy * W + qx];
        if (rq == c || ld_relaxed(m.stamp + rq) >= r) continue;   // own pixel, or not anchored at the start of this round
        const long long l = ld_relaxed(m.ulabel + rq);
        if (l == target) ++count;
        else if (l > target && l < next) next = l;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      count += __shfl_xor(count, o, 64);
      const long long other = __shfl_xor(next, o, 64);
      next = other < next ? other : next;
    }
    if (count > best_count) { best_count = count; best = (int)target; }
    if (next == none) break;
    target = next;
  }
  if (best_count > 0 && lane == 0) {
    st_relaxed(m.ulabel + c, best);
    // nobody reads ulabel[c] before a later round (stamp r hides c from round r), and rounds are separated by a kernel boundary or
    // by the tail kernel's fence + barrier
    st_relaxed(m.stamp + c, r);
    atomicSub(cnt + C_REMAINING, 1);
  }
}

__device__ inline Maps image_maps(int* root, int* size, int* stamp, int* ulabel, int* slice, int* plist, size_t img) {
  Maps m;
  m.root = root + img; m.size = size + img; m.slice = slice + img; m.plist = plist + img; m.stamp = stamp + img; m.ulabel = ulabel + img;
  return m;
}

__global__ __launch_bounds__(256) void round_kernel(int* root, int* size, int* stamp, int* ulabel, int* slice, int* plist,
                                                    const int* __restrict__ wlist, int* cnt, int H, int W, int r) {
  int* c = cnt + blockIdx.y * C_STRIDE;
  // C_REMAINING changes during the kernel; C_NANCH and C_NWAIT do not.  A wave that reads zero here has nothing left to do in this
  // round whatever the others do.
  if (c[C_NANCH] == 0 || ld_relaxed(c + C_REMAINING) == 0) return;
  const size_t img = (size_t)blockIdx.y * H * W;
  const Maps m = image_maps(root, size, stamp, ulabel, slice, plist, img);
  const int nw = c[C_NWAIT], lane = threadIdx.x & 63;
  const int waves = gridDim.x * (blockDim.x / WVN_WAVE);
  for (int w = blockIdx.x * (blockDim.x / WVN_WAVE) + threadIdx.x / WVN_WAVE; w < nw; w += waves)
    decide_component(m, c, wlist[img + w], r, H, W, lane);
}

// Rounds PAR_ROUNDS + 1, ... of one image in one workgroup.  Ends: while the counter is positive and an anchored component exists, the
// connected pixel grid gives some waiting component an anchored neighbour, so every round lowers the counter by at least one; it is
// read once per round by one lane and handed to the others through LDS, so the whole workgroup leaves in the same round.  The round
// number is capped at PAR_ROUNDS + nwait as well (a round that absorbs nothing cannot exist; the cap makes that local to this loop).
__global__ __launch_bounds__(TAIL_THREADS) void tail_kernel(int* root, int* size, int* stamp, int* ulabel, int* slice, int* plist,
                                                            const int* __restrict__ wlist, int* cnt, int H, int W) {
  __shared__ int s_remaining;
  int* c = cnt + blockIdx.x * C_STRIDE;
  if (c[C_NANCH] == 0) {   // nothing is anchored: the map stays as it is (step 2), and nothing is left to decide
    if (threadIdx.x == 0) c[C_REMAINING] = 0;
    return;
  }
  const size_t img = (size_t)blockIdx.x * H * W;
  const Maps m = image_maps(root, size, stamp, ulabel, slice, plist, img);
  const int nw = c[C_NWAIT], lane = threadIdx.x & 63;
  for (int r = PAR_ROUNDS + 1; r <= PAR_ROUNDS + nw; ++r) {
    if (threadIdx.x == 0) s_remaining = ld_relaxed(c + C_REMAINING);
    __syncthreads();
    if (s_remaining == 0) break;
    for (int w = threadIdx.x / WVN_WAVE; w < nw; w += TAIL_THREADS / WVN_WAVE) decide_component(m, c, wlist[img + w], r, H, W, lane);
    __threadfence();
    __syncthreads();   // also keeps lane 0's next write of s_remaining behind every lane's read of it
  }
}

__global__ __launch_bounds__(256) void relabel_kernel(const int* __restrict__ root, const int* __restrict__ ulabel, int* __restrict__ out,
                                                      int npix) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const size_t img = (size_t)blockIdx.y * npix;
  out[img + p] = ulabel[img + root[img + p]];
}

bool conn_shape_ok(int B, int H, int W) {
  // frame indices and the batch offset of an int array are 32-bit quantities in the kernels' grids; blockIdx.y / .z carry the batch
  return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && (long long)H * W <= 0x7fffffffll / 4 && (long long)B * H * W <= 0x7fffffffll / 4;
}
size_t conn_counter_bytes(int B) { return align_up((size_t)B * C_STRIDE * sizeof(int), 256); }
size_t conn_map_bytes(int B, int H, int W) { return align_up((size_t)B * H * W * sizeof(int), 256); }

}  // namespace

size_t wvn_slic_connectivity_scratch_bytes_impl(int B, int H, int W, int K) {
  if (!conn_shape_ok(B, H, W) || K < 1) return 0;
  return conn_counter_bytes(B) + 7 * conn_map_bytes(B, H, W);
}

int wvn_slic_connectivity_launch(const int* labels_in, int* labels_out, int B, int H, int W, int K, int min_size, void* scratch,
                                 size_t scratch_bytes, hipStream_t st) {
  if (!labels_in || !labels_out || !scratch || B < 1 || H < 1 || W < 1 || K < 1 || min_size < 1 || !conn_shape_ok(B, H, W))
    return WVN_ERR_ARG;
  if (scratch_bytes < wvn_slic_connectivity_scratch_bytes_impl(B, H, W, K)) return WVN_ERR_ARG;
  const int npix = H * W;
  const size_t cb = conn_counter_bytes(B), mb = conn_map_bytes(B, H, W);
  char* s = (char*)scratch;
  int* cnt = (int*)s;
  int* size = (int*)(s + cb);          // (counters and sizes are adjacent: one memset clears both)
  int* root = (int*)(s + cb + mb);
  int* stamp = (int*)(s + cb + 2 * mb);
  int* ulabel = (int*)(s + cb + 3 * mb);
  int* slice = (int*)(s + cb + 4 * mb);
  int* wlist = (int*)(s + cb + 5 * mb);
  int* plist = (int*)(s + cb + 6 * mb);
  hipError_t e = hipMemsetAsync(s, 0, cb + mb, st);
  if (e != hipSuccess) return (int)e;
  const dim3 px(ceil_div(npix, 256), B);
  hipLaunchKernelGGL(cc_tile_kernel, dim3(ceil_div(W, TW), ceil_div(H, TH), B), dim3(TW * TH), 0, st, labels_in, root, H, W);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_merge_kernel, px, dim3(256), 0, st, labels_in, root, H, W);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, px, dim3(256), 0, st, root, size, npix);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(classify_kernel, px, dim3(256), 0, st, labels_in, root, size, stamp, ulabel, slice, wlist, cnt, npix, min_size);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(scatter_kernel, px, dim3(256), 0, st, root, stamp, slice, plist, npix);
  WVN_LAUNCH_CHECK();
  // four waves per workgroup, one component per wave at a time; the grid is sized for "a wave per 64 pixels" and strides beyond that
  const dim3 rg(ceil_div(npix, 256) < 1024 ? ceil_div(npix, 256) : 1024, B);
  for (int r = 1; r <= PAR_ROUNDS; ++r) {
    hipLaunchKernelGGL(round_kernel, rg, dim3(256), 0, st, root, size, stamp, ulabel, slice, plist, wlist, cnt, H, W, r);
    WVN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(tail_kernel, dim3(B), dim3(TAIL_THREADS), 0, st, root, size, stamp, ulabel, slice, plist, wlist, cnt, H, W);
  WVN_LAUNCH_CHECK();
  hipLaunchKernelGGL(relabel_kernel, px, dim3(256), 0, st, root, ulabel, labels_out, npix);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
