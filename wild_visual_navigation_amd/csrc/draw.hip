// Vector primitives on the packed RGB canvas of the overlays: what visu/visualizer.py of the reference draws with PIL.ImageDraw
// (plot_traversability_graph, plot_graph_result, plot_optical_flow, plot_sparse_optical_flow) -- a 1-pixel line, a 2-pixel line, a
// filled ellipse in the box of +-5 around a centre -- defined bit for bit against Pillow.  DESIGN.md section 4 "Overlays: vector
// primitives" has the rules; tests/visu_draw_ref.py is the same statement in plain loops and tests/test_visu_draw_host.py holds
// that statement to PIL itself.
//
//   draw_kernel   one workgroup per 16 x 16 pixel tile of one frame, one thread per pixel.  The primitive list is walked in chunks
//                 of 256: a thread prepares one primitive (truncation, validity, bounding box inside its panel, the slope of the
//                 2-pixel parallelogram) and the ones whose box meets the tile are compacted IN INDEX ORDER into LDS (ballot +
//                 prefix count, no atomics); then every pixel walks that short list from its end with closed-form coverage tests
//                 and takes the first hit.  Later chunks overrule earlier ones: a pixel gets the colour of the highest-index
//                 primitive that covers it, uncovered pixels are not written.
//
// Integer arithmetic throughout; fp64 only for the truncation PIL does on doubles (and the ellipse box c -+ 5); fp32, one operation
// at a time (this unit is compiled with -ffp-contract=off), for the polygon scanline of the 2-pixel line, as in Pillow's Draw.c.
// The only atomic is the integer count of skipped primitives.
#include "../../include/wvn_hip.h"

#include "common.h"
#include "wvn_internal.h"

namespace {

constexpr int DR_TILE = 16;
constexpr int DR_THREADS = DR_TILE * DR_TILE;
constexpr int DR_WAVES = DR_THREADS / WVN_WAVE;

struct DrRec {
  int kind;
  unsigned colour;
  int bx0, by0, bx1, by1;   // bounding box in CANVAS coordinates, clipped to the primitive's panel, inclusive (empty: bx0 > bx1)
  int px;                   // first canvas column of the panel
  int g[4];                 // lines: truncated x0, y0, x1, y1 (panel-local); disc: box x0, y0, width, height (9 or 10)
  int ex, ey;               // 2-pixel line: the offsets of the parallelogram, each in {-1, 0, 1}
  float slope;              // 2-pixel line: (float)(x1 - x0) / (y1 - y0) of the two long edges (unused when y0 == y1)
};

// (int) of a double, as PIL casts every coordinate: false when the value is not finite or its truncation leaves [-32768, 32767]
__device__ inline bool dr_trunc(double v, int& out) {
  if (!(__builtin_fabs(v) < __builtin_inf())) return false;
  const double t = __builtin_trunc(v);
  if (t < -32768.0 || t > 32767.0) return false;
  out = (int)t;
  return true;
}

__device__ inline int dr_min(int a, int b) { return a < b ? a : b; }
__device__ inline int dr_max(int a, int b) { return a > b ? a : b; }

// Pillow's ROUND_UP / ROUND_DOWN on a float: half away from / toward zero, symmetric about zero
__device__ inline int dr_round_up(float f) { return f >= 0.f ? (int)floorf(__fadd_rn(f, 0.5f)) : -(int)floorf(__fadd_rn(fabsf(f), 0.5f)); }
__device__ inline int dr_round_down(float f) { return f >= 0.f ? (int)ceilf(__fsub_rn(f, 0.5f)) : -(int)ceilf(__fsub_rn(fabsf(f), 0.5f)); }

// Bresenham's minor-axis steps after i major steps (error 2 minor - major at the start, a step when e >= 0) = floor(minor i / major + 1/2)
__device__ inline int dr_bresenham(int minor, int major, int i) {
  if (major < 32768) return (int)((2u * (unsigned)minor * (unsigned)i + (unsigned)major) / (2u * (unsigned)major));
  return (int)((2ull * (unsigned long long)minor * (unsigned long long)i + (unsigned long long)major) / (2ull * (unsigned long long)major));
}

// ImageDraw.line(width <= 1): line8 / line32 of Draw.c plus the last point -- both ends painted, no endpoint swap
__device__ inline bool dr_cover_thin(int x, int y, int x0, int y0, int x1, int y1) {
  int dx = x1 - x0, dy = y1 - y0;
  const int xs = dx < 0 ? -1 : 1, ys = dy < 0 ? -1 : 1;
  dx *= xs;
  dy *= ys;
  if (dx > dy) {
    const int i = (x - x0) * xs;
    if (i < 0 || i > dx) return false;
    return y == y0 + ys * dr_bresenham(dy, dx, i);
  }
  const int i = (y - y0) * ys;
  if (i < 0 || i > dy) return false;
  return x == x0 + (dy == 0 ? 0 : xs * dr_bresenham(dx, dy, i));
}

// ImageDraw.line(width = 2): ImagingDrawWideLine -> polygon_generic on the four vertices (x0, y0 + ey), (x1, y1 + ey), (x1 + ex, y1),
// (x0 + ex, y0).  Row y: every non-horizontal edge with ymin <= y <= ymax gives x = (y - ya) * slope + xa (fp32, the edge's FIRST
// vertex), twice when y is the edge's last row and not the polygon's; the sorted values are paired and each pair fills
// [ROUND_UP(a), ROUND_DOWN(b)]; horizontal edges are spans of their own.
__device__ inline bool dr_cover_wide(int x, int y, const DrRec& r) {
  const int x0 = r.g[0], y0 = r.g[1], x1 = r.g[2], y1 = r.g[3];
  if (x0 == x1 && y0 == y1) return x == x0 && y == y0;
  const int vx[4] = {x0, x1, x1 + r.ex, x0 + r.ex};
  const int vy[4] = {y0 + r.ey, y1 + r.ey, y1, y0};
  const int poly_ymax = dr_max(dr_max(vy[0], vy[1]), dr_max(vy[2], vy[3]));
  const float short_slope = (float)(-r.ex * r.ey);   // ex / (0 - ey) of edges 1 and 3 (they are horizontal when ey == 0)
  float xx[8];
  int n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xa = vx[k], ya = vy[k], xb = vx[(k + 1) & 3], yb = vy[(k + 1) & 3];
    const int ymin = dr_min(ya, yb), ymax = dr_max(ya, yb);
    if (ya == yb) {
      if (y == ya && x >= dr_min(xa, xb) && x <= dr_max(xa, xb)) return true;
      continue;
    }
    if (y < ymin || y > ymax) continue;
    const float v = __fadd_rn(__fmul_rn((float)(y - ya), (k & 1) ? short_slope : r.slope), (float)xa);
    xx[n++] = v;
    if (y == ymax && y < poly_ymax) xx[n++] = v;
  }
  // insertion sort of at most 8 values
  for (int i = 1; i < n; ++i) {
    const float v = xx[i];
    int j = i - 1;
    while (j >= 0 && xx[j] > v) {
      xx[j + 1] = xx[j];
      --j;
    }
    xx[j + 1] = v;
  }
  for (int i = 1; i < n; i += 2)
    if (x >= dr_round_up(xx[i - 1]) && x <= dr_round_down(xx[i])) return true;
  return false;
}

// ImageDraw.ellipse(box, fill=...) on the truncated box of +-5: width and height are 9 or 10 and each of the four sizes is one fixed
// stamp -- row r of a box h high is inset by max(0, 3 - min(r, h - r)) at both ends
__device__ inline bool dr_cover_disc(int x, int y, const DrRec& r) {
  const int lx = x - r.g[0], ly = y - r.g[1];
  if (lx < 0 || lx > r.g[2] || ly < 0 || ly > r.g[3]) return false;
  return dr_min(lx, r.g[2] - lx) + dr_min(ly, r.g[3] - ly) >= 3;
}

// primitive i -> record; false: skipped (a coordinate that is not finite or truncates outside [-32768, 32767], an unknown kind, a
// frame or panel outside the canvas)
__device__ inline bool dr_setup(const wvn_draw_desc& d, int i, DrRec& r, int& frame) {
  const int kind = d.kinds[i];
  frame = d.frame[i];
  const int panel = d.panel[i];
  r.kind = -1;
  if (kind != WVN_DRAW_LINE && kind != WVN_DRAW_LINE2 && kind != WVN_DRAW_DISC) return false;
  if (frame < 0 || frame >= d.B || panel < 0 || panel >= d.P) return false;
  const float* p = d.points + 4 * (size_t)i;
  int lx0, ly0, lx1, ly1;   // the box of the primitive, panel-local
  r.ex = r.ey = 0;
  r.slope = 0.f;
  if (kind == WVN_DRAW_DISC) {
    const double cx = (double)p[0], cy = (double)p[1];
    int x0, y0, x1, y1;
    if (!dr_trunc(cx - 5.0, x0) || !dr_trunc(cy - 5.0, y0) || !dr_trunc(cx + 5.0, x1) || !dr_trunc(cy + 5.0, y1)) return false;
    r.g[0] = x0; r.g[1] = y0; r.g[2] = x1 - x0; r.g[3] = y1 - y0;
    lx0 = x0; ly0 = y0; lx1 = x1; ly1 = y1;
  } else {
    int x0, y0, x1, y1;
    if (!dr_trunc((double)p[0], x0) || !dr_trunc((double)p[1], y0) || !dr_trunc((double)p[2], x1) || !dr_trunc((double)p[3], y1)) return false;
    r.g[0] = x0; r.g[1] = y0; r.g[2] = x1; r.g[3] = y1;
    lx0 = dr_min(x0, x1); lx1 = dr_max(x0, x1); ly0 = dr_min(y0, y1); ly1 = dr_max(y0, y1);
    if (kind == WVN_DRAW_LINE2 && (x0 != x1 || y0 != y1)) {
      // ROUND_DOWN(dy / hypot(dx, dy)) is sign(dy) when |dy| / hypot > 1/2, i.e. 3 dy^2 > dx^2, else 0 (never a tie for integers)
      const long long dx = x1 - x0, dy = y1 - y0;
      r.ex = 3 * dy * dy > dx * dx ? (dy > 0 ? 1 : -1) : 0;
      r.ey = 3 * dx * dx > dy * dy ? (dx > 0 ? 1 : -1) : 0;
      if (dy != 0) r.slope = __fdiv_rn((float)(x1 - x0), (float)(y1 - y0));
      lx0 = dr_min(lx0, lx0 + r.ex); lx1 = dr_max(lx1, lx1 + r.ex);
      ly0 = dr_min(ly0, ly0 + r.ey); ly1 = dr_max(ly1, ly1 + r.ey);
    }
  }
  r.kind = kind;
  r.colour = (unsigned)d.colours[3 * (size_t)i] | ((unsigned)d.colours[3 * (size_t)i + 1] << 8) | ((unsigned)d.colours[3 * (size_t)i + 2] << 16);
  r.px = panel * d.Wp;
  r.bx0 = r.px + dr_max(lx0, 0);
  r.bx1 = r.px + dr_min(lx1, d.Wp - 1);
  r.by0 = dr_max(ly0, 0);
  r.by1 = dr_min(ly1, d.H - 1);
  return true;
}

// grid (tiles of the [H][P * Wp] canvas, B)
__global__ __launch_bounds__(DR_THREADS) void draw_kernel(const wvn_draw_desc d) {
  __shared__ DrRec list[DR_THREADS];
  __shared__ int wave_count[DR_WAVES];
  const int Wc = d.P * d.Wp;
  const int tiles_x = (Wc + DR_TILE - 1) / DR_TILE;
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x), b = blockIdx.y;
  const int lane = threadIdx.x & (WVN_WAVE - 1), wave = threadIdx.x / WVN_WAVE;
  const int X0 = tx * DR_TILE, Y0 = ty * DR_TILE;
  const int X = X0 + (threadIdx.x & (DR_TILE - 1)), Y = Y0 + (threadIdx.x / DR_TILE);
  const bool counts = d.skipped != nullptr && blockIdx.x == 0 && b == 0;
  bool hit = false;
  unsigned colour = 0u;
  for (int base = 0; base < d.N; base += DR_THREADS) {
    const int i = base + (int)threadIdx.x;
    DrRec r;
    bool keep = false;
    if (i < d.N) {
      int frame;
      const bool valid = dr_setup(d, i, r, frame);
      if (!valid && counts) atomicAdd(d.skipped, 1);
      keep = valid && frame == b && r.bx0 <= r.bx1 && r.by0 <= r.by1 && r.bx0 <= X0 + DR_TILE - 1 && r.bx1 >= X0 &&
             r.by0 <= Y0 + DR_TILE - 1 && r.by1 >= Y0;
    }
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(votes);
    __syncthreads();
    int slot = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < DR_WAVES; ++w) {
      if (w < wave) slot += wave_count[w];
      total += wave_count[w];
    }
    if (keep) list[slot] = r;
    __syncthreads();
    for (int j = total - 1; j >= 0; --j) {
      const DrRec& q = list[j];
      if (X < q.bx0 || X > q.bx1 || Y < q.by0 || Y > q.by1) continue;   // (inside the primitive's own panel and the canvas)
      const int x = X - q.px;
      bool c;
      if (q.kind == WVN_DRAW_LINE) c = dr_cover_thin(x, Y, q.g[0], q.g[1], q.g[2], q.g[3]);
      else if (q.kind == WVN_DRAW_LINE2) c = dr_cover_wide(x, Y, q);
      else c = dr_cover_disc(x, Y, q);
      if (c) {
        hit = true;
        colour = q.colour;
        break;
      }
    }
    // (the next round writes wave_count before its first barrier and the list after it: every reader of this round is past both)
  }
  if (hit) {   // hit implies X < P Wp and Y < H: the boxes are clipped to the canvas
    unsigned char* o = d.canvas + (size_t)b * (size_t)d.frame_bytes + (size_t)Y * (size_t)d.row_bytes + 3 * (size_t)X;
    o[0] = (unsigned char)(colour & 255u);
    o[1] = (unsigned char)((colour >> 8) & 255u);
    o[2] = (unsigned char)((colour >> 16) & 255u);
  }
}

}  // namespace

extern "C" int wvn_draw(const wvn_draw_desc* d, void* stream) {
  if (!d || !d->canvas) return WVN_ERR_ARG;
  if (d->N < 0 || d->N > WVN_DRAW_MAX_PRIMITIVES) return WVN_ERR_ARG;
  if (d->B < 1 || d->B > 65535 || d->P < 1 || d->P > WVN_OVERLAY_MAX_MAPS + 1 || d->H < 1 || d->Wp < 1) return WVN_ERR_ARG;
  const long long Wc = (long long)d->P * d->Wp;
  if (Wc > 0x7fffffffll / 3) return WVN_ERR_ARG;
  if (d->row_bytes < 3 * Wc || d->frame_bytes < 0) return WVN_ERR_ARG;
  if (d->B > 1 && d->frame_bytes < d->row_bytes * (long long)(d->H - 1) + 3 * Wc) return WVN_ERR_ARG;
  const long long tiles = ((Wc + DR_TILE - 1) / DR_TILE) * (((long long)d->H + DR_TILE - 1) / DR_TILE);
  if (tiles > 0x7fffffffll) return WVN_ERR_ARG;
  if (d->N == 0) return WVN_OK;
  if (!d->kinds || !d->points || !d->colours || !d->frame || !d->panel) return WVN_ERR_ARG;
  hipLaunchKernelGGL(draw_kernel, dim3((unsigned)tiles, (unsigned)d->B), dim3(DR_THREADS), 0, (hipStream_t)stream, *d);
  WVN_LAUNCH_CHECK();
  return WVN_OK;
}
