// The code of csrc/supervision.hip's kernel as plain C++: a stand-alone program that runs the kernel's three phases in order on the host,
// so that -fsanitize=address,undefined,float-cast-overflow sees every conversion the kernel makes and each byte it reads or writes
// (tests/test_supervision_host.py builds and runs it; nothing is loaded into Python).  The kernel has barriers, so "every thread in turn"
// would not compute what it computes: instead the per-vertex projection, the closing rule, the per-row scan, the per-row column range and
// the per-pixel merge are inline device functions of supervision.hip, which the kernel calls between its barriers and this program calls
// phase by phase.  The fill walks each row as the kernel's 64 lanes do (x = xa + lane, step 64).  The buffers are heap blocks of exactly
// the size the launcher is told: the point list, the masks, and the [H] + [H] + 2 [N + 1] floats of the kernel's dynamic LDS.
//
//   supervision_host <corpus> <output>
//   corpus: u32 count, then per case 8 x i32 {n, points_batched, N, C, H, W, 0, 0}, f32 value, n x 16 f32 K, n x 16 f32 pose,
//           (points_batched ? n : 1) x N x 3 f32 points, n x C x H x W f32 masks
//   output: per case i32 return code, n x C x H x W f32 masks, n x N x 2 f32 projected, n x N f32 depth
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __device__
#define __forceinline__ inline
#define WVN_OK 0
#define WVN_ERR_ARG 1001

#define WVN_SUPERVISION_HOST_BUILD 1
#include "../wild_visual_navigation_amd/csrc/supervision.hip"

// wvn_project_render_fmin_launch's refusals, then the kernel's body for every node
static int render_on_host(const std::vector<RenderNode>& nodes, const float* points, int points_batched, int N, int C, int H, int W,
                          float value) {
  const int n = (int)nodes.size();
  if (!points || n <= 0 || N < 2 || C <= 0 || H <= 0 || W <= 0) return WVN_ERR_ARG;
  if (!render_fits_lds(H, N)) return WVN_ERR_ARG;
  for (int b = 0; b < n; ++b) {
    float* rows = (float*)malloc(render_lds_bytes(H, N));   // exactly the dynamic LDS of the launch
    float* xl = rows;
    float* xr = rows + H;
    float* px = rows + 2 * H;
    float* py = px + (N + 1);
    const RenderNode nd = nodes[b];
    const float* P = points + (points_batched ? (size_t)b * N * 3 : 0);
    for (int i = 0; i < N; ++i) project_vertex(nd, P, i, px, py);
    const int ne = close_polygon(px, py, N) - 1;
    for (int y = 0; y < H; ++y) scan_row(px, py, ne, y, W, xl[y], xr[y]);
    for (int y = 0; y < H; ++y) {
      const float l = xl[y], r = xr[y];
      int xa, xb;
      if (!row_range(l, r, W, xa, xb)) continue;
      for (int lane = 0; lane < 64; ++lane)
        for (int x = xa + lane; x <= xb; x += 64) merge_pixel(nd.mask, C, H, W, y, x, l, r, value);
    }
    free(rows);
  }
  return WVN_OK;
}

static bool take(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  uint32_t count = 0;
  if (!in || !out || !take(in, &count, 4)) return 2;
  for (uint32_t i = 0; i < count; ++i) {
    int32_t c[8];
    float value;
    if (!take(in, c, sizeof c) || !take(in, &value, 4)) return 2;
    const int n = c[0], batched = c[1], N = c[2], C = c[3], H = c[4], W = c[5];
    if (n <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0) return 2;
    const size_t plane = (size_t)C * H * W;
    std::vector<float> K((size_t)n * 16), pose((size_t)n * 16), pts((size_t)(batched ? n : 1) * N * 3);
    if (!take(in, K.data(), K.size() * 4) || !take(in, pose.data(), pose.size() * 4) || !take(in, pts.data(), pts.size() * 4)) return 2;
    // one heap block per mask, per projected and per depth array: a write one float past any of them is an error
    std::vector<float*> mask(n), proj(n), depth(n);
    std::vector<RenderNode> nodes(n);
    for (int b = 0; b < n; ++b) {
      mask[b] = (float*)malloc(plane * 4);
      proj[b] = (float*)calloc((size_t)N * 2, 4);
      depth[b] = (float*)calloc((size_t)N, 4);
      if (!take(in, mask[b], plane * 4)) return 2;
      nodes[b] = RenderNode{K.data() + 16 * b, pose.data() + 16 * b, mask[b], proj[b], depth[b]};
    }
    const int32_t rc = render_on_host(nodes, pts.data(), batched, N, C, H, W, value);
    fwrite(&rc, 4, 1, out);
    for (int b = 0; b < n; ++b) fwrite(mask[b], 4, plane, out);
    for (int b = 0; b < n; ++b) fwrite(proj[b], 4, (size_t)N * 2, out);
    for (int b = 0; b < n; ++b) fwrite(depth[b], 4, (size_t)N, out);
    for (int b = 0; b < n; ++b) { free(mask[b]); free(proj[b]); free(depth[b]); }
  }
  fclose(in);
  fclose(out);
  return 0;
}
