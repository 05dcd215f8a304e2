// The kernels of csrc/rectify.hip as plain C++: a stand-alone program that runs every thread of every workgroup in turn on the host,
// so that -fsanitize=address,undefined sees each byte the kernels read or write (tests/test_rectify_host.py builds and runs it; nothing
// is loaded into Python).  The few HIP words the file uses are defined here; the buffers are heap blocks of exactly the size the
// entry points are told, so one byte past either end is an error.
//
//   rectify_host <corpus> <output>
//   corpus: u32 count, then per case 12 x i32 {mode (0 unpack, 1 rectify), kind, B, H, W, step, frame_stride, h, w, order, planes, 0},
//           B * frame_stride source bytes and, for mode 1, the two int32 [h][w] map planes
//   output: per case i32 return code, then B * planes * rows * cols bytes (rows x cols = H x W for mode 0, h x w for mode 1)
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct int4 {
  int x, y, z, w;
};
static dim3 blockIdx, threadIdx;
using std::max;
using std::min;
typedef void* hipStream_t;
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define WVN_OK 0
#define WVN_ERR_ARG 1001
#define WVN_LAUNCH_CHECK()
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                 \
  do {                                                                                            \
    const dim3 g_ = (grid), b_ = (block);                                                         \
    (void)(stream);                                                                               \
    for (unsigned bz = 0; bz < g_.z; ++bz)                                                        \
      for (unsigned by = 0; by < g_.y; ++by)                                                      \
        for (unsigned bx = 0; bx < g_.x; ++bx)                                                    \
          for (unsigned ty = 0; ty < b_.y; ++ty)                                                  \
            for (unsigned tx = 0; tx < b_.x; ++tx) {                                              \
              blockIdx = dim3(bx, by, bz);                                                        \
              threadIdx = dim3(tx, ty, 0);                                                        \
              kernel(__VA_ARGS__);                                                                \
            }                                                                                     \
  } while (0)

#define WVN_RECTIFY_HOST_BUILD 1
#include "../wild_visual_navigation_amd/csrc/rectify.hip"

static bool take(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  uint32_t count = 0;
  if (!in || !out || !take(in, &count, 4)) return 2;
  for (uint32_t i = 0; i < count; ++i) {
    int32_t c[12];
    if (!take(in, c, sizeof c)) return 2;
    const int mode = c[0], kind = c[1], B = c[2], H = c[3], W = c[4], step = c[5], stride = c[6], h = c[7], w = c[8], order = c[9], planes = c[10];
    std::vector<uint8_t> src((size_t)B * stride);
    if (!take(in, src.data(), src.size())) return 2;
    const size_t rows = mode ? h : H, cols = mode ? w : W;
    std::vector<uint8_t> dst((size_t)B * planes * rows * cols, 0xA5);
    int32_t rc;
    if (mode == 0) {
      rc = wvn_unpack_frames(src.data(), kind, B, H, W, step, stride, dst.data(), order, nullptr);
    } else {
      std::vector<int32_t> qx(rows * cols), qy(rows * cols);
      if (!take(in, qx.data(), qx.size() * 4) || !take(in, qy.data(), qy.size() * 4)) return 2;
      rc = wvn_rectify_frames(src.data(), kind, B, H, W, step, stride, qx.data(), qy.data(), h, w, dst.data(), order, nullptr);
    }
    fwrite(&rc, 4, 1, out);
    fwrite(dst.data(), 1, dst.size(), out);
  }
  fclose(in);
  fclose(out);
  return 0;
}
