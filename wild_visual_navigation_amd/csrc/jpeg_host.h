// Host stage of the JPEG ingest (include/wvn_hip.h: "JPEG ingest"): parser and sequential Huffman decoder of baseline / extended
// 8-bit JPEG.  Plain C++, no HIP: tests/jpeg_fuzz_main.cpp links jpeg_host.cpp alone under the host sanitizers.
#ifndef WVN_JPEG_HOST_H
#define WVN_JPEG_HOST_H
#include <cstddef>
#include <cstdint>

#include "../../include/wvn_hip.h"

namespace wvn_jpeg {

// block grid of one component, padded to whole MCUs (the layout of the coefficient array and of the component planes)
struct Layout {
  int ncomp;
  int hs[3], vs[3];          // sampling factors
  int mcus_x, mcus_y;
  int bw[3], bh[3];          // blocks per row / column of component c
  int cw[3], ch[3];          // the component's real size in samples: ceil(width hs / hmax), ceil(height vs / vmax)
  long long block0[3];       // first block of component c in the frame's coefficient array
  long long blocks;          // blocks per frame
  long long plane0[3];       // first byte of component c's plane (bw 8 x bh 8 samples)
  long long plane_bytes;     // bytes of the planes of one frame
};

// WVN_JPEG_OK and a filled layout, or WVN_JPEG_BAD_GEOMETRY for a geometry the decoder does not produce (sizes outside
// [1, WVN_JPEG_MAX_DIM], unknown sampling, a component count that does not match the sampling).
int layout_of(const wvn_jpeg_geometry* g, Layout* L);

// Header only: fills *g.  Never reads outside [data, data + n).
int parse_info(const uint8_t* data, size_t n, wvn_jpeg_geometry* g);

// Geometry of every frame of a batch in one pass: markers and segment lengths are walked up to SOS, Huffman codes are not built (a
// table that is wrong shows in the decode).  status[b] != WVN_JPEG_OK: g[b] is all zero.
void probe_batch(const void* const* data, const size_t* sizes, int B, wvn_jpeg_geometry* g, int* status);

// Whole frame: quantised coefficients in natural order, int16 [L.blocks][64], and the quantisation tables of the components in
// natural order, uint16 [3][64] (a grayscale frame fills table 0, the others are zero).  `expect` is the geometry the arrays were
// sized for: a frame of another geometry is WVN_JPEG_GEOMETRY_MISMATCH.  On any status but WVN_JPEG_OK both arrays are all zero.
int decode_coefficients(const uint8_t* data, size_t n, const wvn_jpeg_geometry* expect, int16_t* coef, uint16_t* qt);

// frames [0, B) on min(threads, B, WVN_JPEG_MAX_THREADS) workers; coef + b * coef_stride (int16 elements), qt + b * qt_stride (uint16 elements)
void decode_batch_host(const void* const* data, const size_t* sizes, int B, const wvn_jpeg_geometry* g, int16_t* coef, size_t coef_stride,
                       uint16_t* qt, size_t qt_stride, int threads, int* status);

}  // namespace wvn_jpeg
#endif
