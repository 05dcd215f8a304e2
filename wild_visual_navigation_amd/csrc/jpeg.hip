// Device stage of the JPEG ingest (include/wvn_hip.h: "JPEG ingest") and its C entry points.  The host stage (jpeg_host.cpp) hands
// over quantised coefficients; here: dequantise + libjpeg's "islow" inverse DCT to component planes, then fancy chroma upsampling +
// YCbCr -> RGB per output pixel.  Integers only, every operation in 32 bits.  The host stage lets through only frames whose values stay
// in the range where libjpeg's C and SIMD code agree (WVN_JPEG_OUT_OF_RANGE otherwise); there 32-bit arithmetic is exact as well, so
// the frame is libjpeg's bit for bit.  The arithmetic is unsigned where a signed overflow would be undefined: a frame that failed on
// the host still passes through the first kernel (its coefficients are zero) before the second writes it as zeros.
// Both kernels move bytes and do little else: 2 B in and 1 B out per sample in the first, ~1.5 B in and 3 B out per pixel in the second.
#include <mutex>

#include "common.h"
#include "jpeg_host.h"
#include "wvn_internal.h"

namespace {

using wvn_jpeg::Layout;

constexpr int META_BYTES = 512;    // per frame: uint16 q[3][64] (natural order), then uint16 valid, padding
constexpr int META_VALID = 192;
constexpr int IDCT_BLOCKS = 32;    // 8 x 8 blocks per workgroup, 8 threads each

struct DevLayout {
  int ncomp, sampling, width, height;
  int bw[3], bh[3], cw[3], ch[3];
  long long block0[3], plane0[3];
  long long blocks, plane_bytes, up_stride;
};

// one 8-point pass of jidctint.c (jpeg_idct_islow): the same butterfly serves columns and rows, they differ in the descale
__device__ __forceinline__ void islow_1d(const int* in, int* out, int shift) {
  typedef unsigned U;
  U z2 = (U)in[2], z3 = (U)in[6];
  U z1 = (z2 + z3) * 4433u;
  U tmp2 = z1 + z3 * (U)(-15137);
  U tmp3 = z1 + z2 * 6270u;
  z2 = (U)in[0];
  z3 = (U)in[4];
  U tmp0 = (z2 + z3) << 13;
  U tmp1 = (z2 - z3) << 13;
  const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = (U)in[7];
  tmp1 = (U)in[5];
  tmp2 = (U)in[3];
  tmp3 = (U)in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  U z4 = tmp1 + tmp3;
  const U z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u;
  tmp1 *= 16819u;
  tmp2 *= 25172u;
  tmp3 *= 12299u;
  z1 *= (U)(-7373);
  z2 *= (U)(-20995);
  z3 *= (U)(-16069);
  z4 *= (U)(-3196);
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const U half = 1u << (shift - 1);
  out[0] = (int)(tmp10 + tmp3 + half) >> shift;
  out[7] = (int)(tmp10 - tmp3 + half) >> shift;
  out[1] = (int)(tmp11 + tmp2 + half) >> shift;
  out[6] = (int)(tmp11 - tmp2 + half) >> shift;
  out[2] = (int)(tmp12 + tmp1 + half) >> shift;
  out[5] = (int)(tmp12 - tmp1 + half) >> shift;
  out[3] = (int)(tmp13 + tmp0 + half) >> shift;
  out[4] = (int)(tmp13 - tmp0 + half) >> shift;
}

// libjpeg's range_limit[(x) & RANGE_MASK] behind the IDCT: x taken as a 10-bit signed number, + 128, clamped
__device__ __forceinline__ unsigned idct_limit(int x) {
  int v = x & 1023;
  if (v >= 512) v -= 1024;
  v += 128;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// 8 threads per block: thread j loads row j (16 B), runs column j of pass 1 and row j of pass 2, stores 8 samples (8 B).
__global__ __launch_bounds__(IDCT_BLOCKS * 8) void jpeg_idct_kernel(const unsigned char* __restrict__ up, unsigned char* __restrict__ planes,
                                                                    DevLayout L, long long total_blocks) {
  __shared__ int ws[IDCT_BLOCKS][8][9];
  const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
  const long long gb = (long long)blockIdx.x * IDCT_BLOCKS + lb;
  const bool live = gb < total_blocks;
  int c = 0, bx = 0, by = 0;
  long long b = 0;
  if (live) {
    b = gb / L.blocks;
    const long long i = gb - b * L.blocks;
    c = (L.ncomp == 3 && i >= L.block0[1]) ? (i >= L.block0[2] ? 2 : 1) : 0;
    const int li = (int)(i - L.block0[c]);
    by = li / L.bw[c];
    bx = li - by * L.bw[c];
    const unsigned char* frame = up + b * L.up_stride;
    const uint4 cv = *reinterpret_cast<const uint4*>(frame + META_BYTES + (i * 64 + j * 8) * 2);
    const uint4 qv = *reinterpret_cast<const uint4*>(frame + (c * 64 + j * 8) * 2);
    const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c0 = (int)(short)(cw[k] & 0xffffu), c1 = (int)(short)(cw[k] >> 16);
      ws[lb][j][2 * k] = (int)((unsigned)c0 * (qw[k] & 0xffffu));
      ws[lb][j][2 * k + 1] = (int)((unsigned)c1 * (qw[k] >> 16));
    }
  }
  __syncthreads();
  int in[8], out[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) in[k] = ws[lb][k][j];
  islow_1d(in, out, 13 - 2);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) ws[lb][k][j] = out[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) in[k] = ws[lb][j][k];
  islow_1d(in, out, 13 + 2 + 3);
  if (live) {
    uint2 o;
    o.x = idct_limit(out[0]) | (idct_limit(out[1]) << 8) | (idct_limit(out[2]) << 16) | (idct_limit(out[3]) << 24);
    o.y = idct_limit(out[4]) | (idct_limit(out[5]) << 8) | (idct_limit(out[6]) << 16) | (idct_limit(out[7]) << 24);
    unsigned char* plane = planes + b * L.plane_bytes + L.plane0[c];
    *reinterpret_cast<uint2*>(plane + ((long long)(by * 8 + j) * L.bw[c] + bx) * 8) = o;
  }
}

// h2v1 fancy upsampling of one row s (real width cw) at output column x
__device__ __forceinline__ int up_h2v1(const unsigned char* s, int cw, int x) {
  const int i = x >> 1;
  if (cw <= 2) return s[i];
  const int v = s[i];
  if (x & 1) return i == cw - 1 ? v : (3 * v + s[i + 1] + 2) >> 2;
  return i == 0 ? v : (3 * v + s[i - 1] + 1) >> 2;
}

// h2v2: `near` the chroma row of this output row, `far` the one above (even output rows) or below (odd), clamped to the real rows
__device__ __forceinline__ int up_h2v2(const unsigned char* near, const unsigned char* far, int cw, int x) {
  const int i = x >> 1;
  if (cw <= 2) return near[i];
  const int t = 3 * near[i] + far[i];
  if (x & 1) return i == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
  return i == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// one thread: 4 pixels of one row
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const unsigned char* __restrict__ up, const unsigned char* __restrict__ planes,
                                                          unsigned char* __restrict__ out, DevLayout L, int out_ch) {
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int y = blockIdx.y * 4 + threadIdx.y;
  const long long b = blockIdx.z;
  const int W = L.width, H = L.height;
  if (x0 >= W || y >= H) return;
  const bool valid = reinterpret_cast<const unsigned short*>(up + b * L.up_stride)[META_VALID] != 0;
  const unsigned char* P = planes + b * L.plane_bytes;
  unsigned rgb[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  if (valid) {
    const unsigned char* yrow = P + L.plane0[0] + (long long)y * (L.bw[0] * 8);
    const unsigned char *b0 = nullptr, *b1 = nullptr, *r0 = nullptr, *r1 = nullptr;
    if (L.ncomp == 3) {
      const int pw = L.bw[1] * 8;
      int rn = y, rf = y;
      if (L.sampling == WVN_JPEG_420) {
        rn = y >> 1;
        rf = (y & 1) ? min(rn + 1, L.ch[1] - 1) : max(rn - 1, 0);
      }
      b0 = P + L.plane0[1] + (long long)rn * pw;
      b1 = P + L.plane0[1] + (long long)rf * pw;
      r0 = P + L.plane0[2] + (long long)rn * pw;
      r1 = P + L.plane0[2] + (long long)rf * pw;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      if (x >= W) break;
      const int Y = yrow[x];
      if (L.ncomp == 1) {
        rgb[0][k] = rgb[1][k] = rgb[2][k] = (unsigned)Y;
        continue;
      }
      int cb, cr;
      if (L.sampling == WVN_JPEG_444) {
        cb = b0[x];
        cr = r0[x];
      } else if (L.sampling == WVN_JPEG_422) {
        cb = up_h2v1(b0, L.cw[1], x);
        cr = up_h2v1(r0, L.cw[1], x);
      } else {
        cb = up_h2v2(b0, b1, L.cw[1], x);
        cr = up_h2v2(r0, r1, L.cw[1], x);
      }
      cb -= 128;
      cr -= 128;
      rgb[0][k] = clamp255(Y + ((91881 * cr + 32768) >> 16));
      rgb[1][k] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      rgb[2][k] = clamp255(Y + ((116130 * cb + 32768) >> 16));
    }
  }
  for (int c = 0; c < out_ch; ++c) {
    unsigned char* o = out + ((b * out_ch + c) * H + y) * (long long)W + x0;
    if ((W & 3) == 0) {
      *reinterpret_cast<unsigned*>(o) = rgb[c][0] | (rgb[c][1] << 8) | (rgb[c][2] << 16) | (rgb[c][3] << 24);
    } else {
      for (int k = 0; k < 4 && x0 + k < W; ++k) o[k] = (unsigned char)rgb[c][k];
    }
  }
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

int dev_layout(const wvn_jpeg_geometry* g, DevLayout* D) {
  Layout L;
  if (!g || wvn_jpeg::layout_of(g, &L) != WVN_JPEG_OK) return WVN_ERR_ARG;
  D->ncomp = L.ncomp;
  D->sampling = g->sampling;
  D->width = g->width;
  D->height = g->height;
  for (int c = 0; c < 3; ++c) {
    D->bw[c] = L.bw[c];
    D->bh[c] = L.bh[c];
    D->cw[c] = L.cw[c];
    D->ch[c] = L.ch[c];
    D->block0[c] = L.block0[c];
    D->plane0[c] = L.plane0[c];
  }
  D->blocks = L.blocks;
  D->plane_bytes = L.plane_bytes;
  D->up_stride = META_BYTES + L.blocks * 128;
  return WVN_OK;
}

// Pinned staging, reused across calls: two buffers alternate, each with the event recorded behind its last upload.
struct Slot {
  void* host = nullptr;
  size_t bytes = 0;
  hipEvent_t uploaded = nullptr;
};
std::mutex g_mu;
Slot g_slot[2];
int g_next = 0;

}  // namespace

extern "C" {

int wvn_jpeg_info(const void* data, size_t n, wvn_jpeg_geometry* out) {
  if (!data || !out) return WVN_ERR_ARG;
  return wvn_jpeg::parse_info((const uint8_t*)data, n, out);
}

int wvn_jpeg_probe_batch(const void* const* data, const size_t* sizes, int B, wvn_jpeg_geometry* g, int* status) {
  if (!data || !sizes || !g || !status || B < 1 || B > WVN_JPEG_MAX_BATCH) return WVN_ERR_ARG;
  for (int b = 0; b < B; ++b)
    if (!data[b]) return WVN_ERR_ARG;
  wvn_jpeg::probe_batch(data, sizes, B, g, status);
  return WVN_OK;
}

size_t wvn_jpeg_coef_bytes(const wvn_jpeg_geometry* g) {
  DevLayout D;
  return dev_layout(g, &D) ? 0 : (size_t)D.blocks * 128;
}

size_t wvn_jpeg_plane_bytes(const wvn_jpeg_geometry* g) {
  DevLayout D;
  return dev_layout(g, &D) ? 0 : (size_t)D.plane_bytes;
}

size_t wvn_jpeg_workspace_bytes(const wvn_jpeg_geometry* g, int B) {
  DevLayout D;
  if (dev_layout(g, &D) || B < 1 || B > WVN_JPEG_MAX_BATCH) return 0;
  return align256((size_t)B * D.up_stride) + align256((size_t)B * D.plane_bytes);
}

int wvn_jpeg_coefficients(const void* data, size_t n, const wvn_jpeg_geometry* g, short* coef, size_t coef_bytes, unsigned short* qtables) {
  const size_t need = wvn_jpeg_coef_bytes(g);
  if (!data || !coef || !qtables || need == 0) return WVN_ERR_ARG;
  if (coef_bytes < need) return WVN_ERR_WORKSPACE;
  return wvn_jpeg::decode_coefficients((const uint8_t*)data, n, g, coef, qtables);
}

int wvn_jpeg_coefficients_batch(const void* const* data, const size_t* sizes, int B, const wvn_jpeg_geometry* g, short* coef,
                                size_t coef_bytes, unsigned short* qtables, int threads, int* status) {
  const size_t one = wvn_jpeg_coef_bytes(g);
  if (!data || !sizes || !coef || !qtables || !status || one == 0 || B < 1 || B > WVN_JPEG_MAX_BATCH) return WVN_ERR_ARG;
  if (coef_bytes / one < (size_t)B) return WVN_ERR_WORKSPACE;
  for (int b = 0; b < B; ++b)
    if (!data[b]) return WVN_ERR_ARG;
  wvn_jpeg::decode_batch_host(data, sizes, B, g, coef, one / 2, qtables, 192, threads, status);
  return WVN_OK;
}

int wvn_jpeg_device_stage(const wvn_jpeg_geometry* g, int B, void* workspace, void* out_u8, int gray_out, void* stream) {
  DevLayout D;
  if (!workspace || !out_u8 || B < 1 || B > WVN_JPEG_MAX_BATCH || dev_layout(g, &D)) return WVN_ERR_ARG;
  if (gray_out && D.ncomp != 1) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* dev_up = (unsigned char*)workspace;
  unsigned char* dev_planes = dev_up + align256((size_t)B * D.up_stride);
  const long long total = (long long)B * D.blocks;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total + IDCT_BLOCKS - 1) / IDCT_BLOCKS)), dim3(IDCT_BLOCKS * 8), 0, st, dev_up,
                     dev_planes, D, total);
  WVN_LAUNCH_CHECK();
  const int out_ch = gray_out ? 1 : 3;
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((D.width + 255) / 256), (unsigned)((D.height + 3) / 4), (unsigned)B),
                     dim3(64, 4), 0, st, dev_up, dev_planes, (unsigned char*)out_u8, D, out_ch);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}

int wvn_jpeg_decode_batch(const void* const* data, const size_t* sizes, int B, const wvn_jpeg_geometry* g, void* out_u8, int gray_out,
                          void* workspace, int threads, int* status, void* stream) {
  DevLayout D;
  if (!data || !sizes || !out_u8 || !workspace || !status || B < 1 || B > WVN_JPEG_MAX_BATCH || dev_layout(g, &D)) return WVN_ERR_ARG;
  if (gray_out && D.ncomp != 1) return WVN_ERR_ARG;
  for (int b = 0; b < B; ++b)
    if (!data[b]) return WVN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t up_bytes = (size_t)B * D.up_stride;
  hipError_t e;

  std::lock_guard<std::mutex> lock(g_mu);
  Slot& s = g_slot[g_next];
  g_next ^= 1;
  if (s.uploaded) {   // the upload that last read this buffer
    e = hipEventSynchronize(s.uploaded);
    (void)hipEventDestroy(s.uploaded);
    s.uploaded = nullptr;
    if (e != hipSuccess) return (int)e;
  }
  if (s.bytes < up_bytes) {
    if (s.host) (void)hipHostFree(s.host);
    s.host = nullptr;
    s.bytes = 0;
    if ((e = hipHostMalloc(&s.host, up_bytes, hipHostMallocPortable)) != hipSuccess) return (int)e;
    s.bytes = up_bytes;
  }
  unsigned char* host = (unsigned char*)s.host;
  wvn_jpeg::decode_batch_host(data, sizes, B, g, (int16_t*)(host + META_BYTES), (size_t)D.up_stride / 2, (uint16_t*)host,
                              (size_t)D.up_stride / 2, threads, status);
  for (int b = 0; b < B; ++b) {
    uint16_t* meta = (uint16_t*)(host + (size_t)b * D.up_stride);
    for (int k = META_VALID; k < META_BYTES / 2; ++k) meta[k] = 0;
    meta[META_VALID] = status[b] == WVN_JPEG_OK ? 1 : 0;
  }
  unsigned char* dev_up = (unsigned char*)workspace;
  if ((e = hipMemcpyAsync(dev_up, host, up_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
  if ((e = hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming)) != hipSuccess) {
    s.uploaded = nullptr;
    (void)hipStreamSynchronize(st);   // without an event the buffer is only safe once the copy is over
    return (int)e;
  }
  if ((e = hipEventRecord(s.uploaded, st)) != hipSuccess) {
    (void)hipEventDestroy(s.uploaded);
    s.uploaded = nullptr;
    (void)hipStreamSynchronize(st);
    return (int)e;
  }
  return wvn_jpeg_device_stage(g, B, workspace, out_u8, gray_out, stream);
}

}  // extern "C"
