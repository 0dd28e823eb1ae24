// Antialiased bicubic resize of uint8 HWC images to ANY size (gfx950): Pillow's Image.resize(..., BICUBIC) byte for byte,
// both passes in one launch, all arithmetic int32.
//
// Definition (image_utils.resize_u8 is the host restatement, image_utils.resize_coeffs makes the tables).  Per axis a
// table pair: bounds [n_out][2] = (lo, n) and coeffs [n_out][ksize], ksize = 2 ceil(2 max(n_in / n_out, 1)) + 1 <= 17 for
// n_in <= 4 n_out; one pass is out[i] = clamp((2^21 + sum_{j < n} in[lo + j] coeffs[i][j]) >> 22, 0, 255).  The horizontal
// pass runs first and leaves BYTES (Pillow's uint8 intermediate: rounded and clamped there), then the vertical one.  An
// axis whose size does not change has no table (ksize 0) and is the identity (lo = i, n = 1, weight 2^22: the same code).
//
// Kernel.  A 256-thread workgroup owns kResizeRows x kResizeCols output pixels of one image:
//   1. the bounds of its first and last output row / column give the source rows [r0, r0 + nrows) and columns [c0, c0 +
//      ncols) it needs (resize_window bounds them: 78 rows, 142 pixels at the largest ratio).  Its slices of the four
//      tables go to LDS, lo made relative to r0 / c0.
//   2. stage: the 3 ncols bytes of every needed source row as ALIGNED dwords, the row keeping the offset of its first
//      byte (skew = address & 3: a row of 3 W bytes has no alignment of its own).  A dword that is not wholly inside the
//      batch (the first / last of the allocation) is put together from guarded byte loads.  A thread issues eight loads
//      before its first LDS store: one memory latency per eight dwords, and one per tile at the usual ratios.
//   3. horizontal pass: item = (source row, output pixel), its three channels share the weights; bytes go to mid[row],
//      4 bytes in: the front pad lets the vertical pass read one dword to the left.
//   4. vertical pass: item = (output row, ALIGNED dword of that output row in global memory): the four bytes start at
//      tile byte 4 d - (row address & 3), two mid dwords + v_alignbyte per tap, one dword store; the ragged ends of a
//      row store bytes.
// LDS: 3.6 KiB of tables, and stage + mid sized by the launch for its ratios (dynamic): rows x (stage pitch + 27) dwords,
// rows = ceil(15 ry) + ceil(4 max(ry, 1)) + 2, stage pitch = the dwords of ceil(31 rx) + ceil(4 max(rx, 1)) + 2 pixels at any
// skew, made odd.  At ratio 4 on both axes that is 78 x (109 + 27) dwords = 45 KiB, three workgroups per CU; at 1.26
// (1356 x 2040 -> 1080 x 1620) 27 x (37 + 27) dwords = 10 KiB, and the CU's eight workgroup slots are all taken.  Banks:
// table rows have pitch 17, stage and mid rows an odd pitch; the 32 lanes of a half-wave are consecutive pixels of a row.
// Every output byte depends on its own coordinates only.  Every LDS index is clamped to what was staged, so a table that
// disagrees with the shapes gives wrong bytes, never an access outside the tile or the images.
#include "larva_common.h"

namespace larva {

constexpr int kResizeRows = 16;    // output rows of a tile (kernels.RESIZE_TILE_ROWS / RESIZE_TILE_COLS mirror these)
constexpr int kResizeCols = 32;    // output pixels of a tile row
constexpr int kResizeTaps = 17;    // largest ksize: n_in <= 4 n_out
constexpr int kResizeBits = 22;
constexpr int kRsSrcRows = 4 * kResizeRows + 16;
constexpr int kRsSrcCols = 4 * kResizeCols + 16;
constexpr int kRsStageBatch = 8;                              // loads a thread has in flight while staging
constexpr int kRsMidPitch = 27;                               // 1 pad + 24 + 2 dwords
constexpr int kRsOutDwords = 3 * kResizeCols / 4 + 1;         // aligned dwords that can hold a tile row's 96 bytes
static_assert(kRsMidPitch % 2 == 1, "odd LDS pitch");

// Source rows (T = kResizeRows) or pixels (T = kResizeCols) a tile can need along an axis: its first and last centres are
// (T - 1) n_in / n_out apart and a window reaches support + 1/2 = 2 max(n_in / n_out, 1) + 1/2 to either side.
__host__ __device__ constexpr int resize_window(int n_in, int n_out, int T) {
  const long long step = ((long long)(T - 1) * n_in + n_out - 1) / n_out;
  const long long reach = n_in > n_out ? (4ll * n_in + n_out - 1) / n_out : 4;
  const long long need = step + reach + 2;
  return (int)(need < n_in ? need : n_in);
}
static_assert(resize_window(4 << 10, 1 << 10, kResizeRows) <= kRsSrcRows && resize_window(4 << 10, 1 << 10, kResizeCols) <= kRsSrcCols,
              "the windows at ratio 4");
static_assert(4 * (kRsOutDwords + 1) <= 4 * kRsMidPitch, "the vertical pass reads mid dwords q and q + 1");

// (lo, n) of output i: from the table, or the identity of a skipped axis; clamped to the axis and to ksize.
__device__ __forceinline__ void resize_bound(const int* __restrict__ bounds, int ksize, int i, int n_in, int& lo, int& n) {
  if (ksize == 0) {
    lo = i;
    n = 1;
  } else {
    lo = bounds[2 * i];
    n = bounds[2 * i + 1];
    n = min(n, ksize);
  }
  lo = min(max(lo, 0), n_in - 1);
  n = min(max(n, 0), n_in - lo);
}

__device__ __forceinline__ unsigned resize_clip(int acc) {
  const int v = acc >> kResizeBits;   // arithmetic
  return (unsigned)min(max(v, 0), 255);
}

__global__ __launch_bounds__(256) void resize_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                        int H, int W, int h, int w, const int* __restrict__ hbounds,
                                                        const int* __restrict__ hcoeffs, int kx,
                                                        const int* __restrict__ vbounds, const int* __restrict__ vcoeffs,
                                                        int ky, int max_rows, int max_cols, int stage_pitch) {
  extern __shared__ unsigned resize_lds[];   // stage [max_rows][stage_pitch], then mid [max_rows][kRsMidPitch]
  unsigned* const stage = resize_lds;
  unsigned* const mid = resize_lds + max_rows * stage_pitch;
  __shared__ int hlo[kResizeCols], hn[kResizeCols], hcs[kResizeCols * kResizeTaps];
  __shared__ int vlo[kResizeRows], vn[kResizeRows], vcs[kResizeRows * kResizeTaps];

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kResizeCols, y0 = blockIdx.y * kResizeRows;
  const int nx = min(kResizeCols, w - x0), ny = min(kResizeRows, h - y0);
  const long long in_bytes = 3ll * H * W;
  const unsigned char* img = src + (long long)blockIdx.z * in_bytes;
  const unsigned char* src_end = src + (long long)gridDim.z * in_bytes;
  unsigned char* out = dst + (long long)blockIdx.z * (3ll * h * w);

  // 1. the source window (uniform) and the tile's tables
  int c0, r0, ncols, nrows;
  {
    int lo, n;
    resize_bound(hbounds, kx, x0, W, c0, n);
    resize_bound(hbounds, kx, x0 + nx - 1, W, lo, n);
    ncols = min(max(lo + n - c0, 0), max_cols);
    resize_bound(vbounds, ky, y0, H, r0, n);
    resize_bound(vbounds, ky, y0 + ny - 1, H, lo, n);
    nrows = min(max(lo + n - r0, 0), max_rows);
  }
  if (tid < kResizeCols + kResizeRows) {
    const bool horiz = tid < kResizeCols;
    const int i = horiz ? tid : tid - kResizeCols;
    if (i < (horiz ? nx : ny)) {
      int lo, n;
      if (horiz) resize_bound(hbounds, kx, x0 + i, W, lo, n); else resize_bound(vbounds, ky, y0 + i, H, lo, n);
      const int first = horiz ? c0 : r0, count = horiz ? ncols : nrows;
      lo = min(max(lo - first, 0), count);
      n = min(n, count - lo);
      if (horiz) { hlo[i] = lo; hn[i] = n; } else { vlo[i] = lo; vn[i] = n; }
    }
  }
  for (int t = tid; t < (kResizeCols + kResizeRows) * kResizeTaps; t += 256) {
    const bool horiz = t < kResizeCols * kResizeTaps;
    const int u = horiz ? t : t - kResizeCols * kResizeTaps;
    const int i = u / kResizeTaps, j = u - i * kResizeTaps;
    const int k = horiz ? kx : ky;
    int c = 0;
    if (i < (horiz ? nx : ny)) {
      if (k == 0) c = 1 << kResizeBits;
      else if (j < k) c = horiz ? hcoeffs[(long long)(x0 + i) * k + j] : vcoeffs[(long long)(y0 + i) * k + j];
    }
    if (horiz) hcs[u] = c; else vcs[u] = c;
  }

  // 2. stage the source window
  const long long pitch = 3ll * W;
  const unsigned char* win = img + (long long)r0 * pitch + 3ll * c0;   // byte 0 of staged row 0
  const int nbytes = 3 * ncols;
  const int ndw = (nbytes + 3 + 3) / 4;   // dwords of a row at any skew: <= stage_pitch
  const float ndw_inv = 1.0f / (float)ndw;
  for (int e0 = tid; e0 < nrows * ndw; e0 += 256 * kRsStageBatch) {
    unsigned held[kRsStageBatch];
#pragma unroll
    for (int k = 0; k < kRsStageBatch; ++k) {
      const int e = e0 + 256 * k;
      const int r = (int)(((float)e + 0.5f) * ndw_inv), d = e - r * ndw;   // e / ndw: e < 2^14, never near a whole number
      held[k] = 0;
      if (e < nrows * ndw) {
        const unsigned char* p = win + (long long)r * pitch;
        const int skew = (int)(reinterpret_cast<uintptr_t>(p) & 3);
        if (4 * d < skew + nbytes) {
          const unsigned char* a = p - skew + 4 * d;
          if (a >= src && a + 4 <= src_end) {
            held[k] = *reinterpret_cast<const unsigned*>(a);
          } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if (a + b >= p && a + b < p + nbytes) held[k] |= (unsigned)a[b] << (8 * b);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kRsStageBatch; ++k) {
      const int e = e0 + 256 * k;
      const int r = (int)(((float)e + 0.5f) * ndw_inv), d = e - r * ndw;
      if (e < nrows * ndw) stage[r * stage_pitch + d] = held[k];
    }
  }
  __syncthreads();

  // 3. horizontal pass -> mid (bytes)
  for (int it = tid; it < nrows * kResizeCols; it += 256) {
    const int r = it / kResizeCols, px = it - r * kResizeCols;
    if (px < nx) {
      const int skew = (int)(reinterpret_cast<uintptr_t>(win + (long long)r * pitch) & 3);
      const unsigned char* sb = reinterpret_cast<const unsigned char*>(stage) + r * (4 * stage_pitch) + skew + 3 * hlo[px];
      const int n = hn[px];
      const int* cf = hcs + px * kResizeTaps;
      int a0 = 1 << (kResizeBits - 1), a1 = a0, a2 = a0;
      for (int j = 0; j < n; ++j) {
        const int c = cf[j];
        a0 += (int)sb[3 * j] * c;
        a1 += (int)sb[3 * j + 1] * c;
        a2 += (int)sb[3 * j + 2] * c;
      }
      unsigned char* mb = reinterpret_cast<unsigned char*>(mid) + r * (4 * kRsMidPitch) + 4 + 3 * px;
      mb[0] = (unsigned char)resize_clip(a0);
      mb[1] = (unsigned char)resize_clip(a1);
      mb[2] = (unsigned char)resize_clip(a2);
    }
  }
  __syncthreads();

  // 4. vertical pass -> global
  const int nb = 3 * nx;
  for (int it = tid; it < kResizeRows * kRsOutDwords; it += 256) {
    const int oy = it / kRsOutDwords, d = it - oy * kRsOutDwords;
    if (oy >= ny) continue;
    unsigned char* row = out + ((long long)(y0 + oy) * w + x0) * 3;
    const int e0 = 4 * d - (int)(reinterpret_cast<uintptr_t>(row) & 3);   // tile byte of this dword's byte 0: >= -3
    if (e0 >= nb) continue;
    const int m0 = e0 + 4, q = m0 >> 2;
    const unsigned sh = (unsigned)(m0 & 3);
    const int n = vn[oy];
    const unsigned* mp = mid + vlo[oy] * kRsMidPitch + q;
    const int* cf = vcs + oy * kResizeTaps;
    int a0 = 1 << (kResizeBits - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int k = 0; k < n; ++k) {
      const unsigned v = __builtin_amdgcn_alignbyte(mp[k * kRsMidPitch + 1], mp[k * kRsMidPitch], sh);
      const int c = cf[k];
      a0 += (int)(v & 255u) * c;
      a1 += (int)((v >> 8) & 255u) * c;
      a2 += (int)((v >> 16) & 255u) * c;
      a3 += (int)(v >> 24) * c;
    }
    const unsigned b0 = resize_clip(a0), b1 = resize_clip(a1), b2 = resize_clip(a2), b3 = resize_clip(a3);
    if (e0 >= 0 && e0 + 4 <= nb) {
      *reinterpret_cast<unsigned*>(row + e0) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    } else {
      if (e0 >= 0 && e0 < nb) row[e0] = (unsigned char)b0;
      if (e0 + 1 >= 0 && e0 + 1 < nb) row[e0 + 1] = (unsigned char)b1;
      if (e0 + 2 >= 0 && e0 + 2 < nb) row[e0 + 2] = (unsigned char)b2;
      if (e0 + 3 < nb) row[e0 + 3] = (unsigned char)b3;
    }
  }
}

// ksize of image_utils.resize_coeffs for one axis, in integers: 2 ceil(2 max(n_in / n_out, 1)) + 1
static int resize_ksize(int n_in, int n_out) {
  const int support_up = n_in > n_out ? (int)((2ll * n_in + n_out - 1) / n_out) : 2;
  return 2 * support_up + 1;
}

}  // namespace larva

using namespace larva;

extern "C" {

int larva_resize_u8(const unsigned char* src, unsigned char* dst, int N, int H, int W, int h, int w, const int* hbounds,
                    const int* hcoeffs, int kx, const int* vbounds, const int* vcoeffs, int ky, void* stream) {
  constexpr int kMaxSide = 1 << 20;
  if (!src || !dst || N < 1 || N > 65535 || H < 1 || W < 1 || h < 1 || w < 1 || H > kMaxSide || W > kMaxSide ||
      h > kMaxSide || w > kMaxSide || H > 4ll * h || W > 4ll * w)
    return (int)hipErrorInvalidValue;
  // an axis without a table keeps its size; one with a table has the ksize of its ratio
  if (kx == 0 ? W != w : (!hbounds || !hcoeffs || kx != resize_ksize(W, w) || kx > kResizeTaps))
    return (int)hipErrorInvalidValue;
  if (ky == 0 ? H != h : (!vbounds || !vcoeffs || ky != resize_ksize(H, h) || ky > kResizeTaps))
    return (int)hipErrorInvalidValue;
  const dim3 grid((w + kResizeCols - 1) / kResizeCols, (h + kResizeRows - 1) / kResizeRows, N), block(256);
  if (grid.y > 65535u) return (int)hipErrorInvalidValue;
  const int max_rows = resize_window(H, h, kResizeRows), max_cols = resize_window(W, w, kResizeCols);
  const int stage_pitch = ((3 * max_cols + 3 + 3) / 4) | 1;
  if (max_rows > kRsSrcRows || max_cols > kRsSrcCols) return (int)hipErrorInvalidValue;   // (unreachable below ratio 4)
  const size_t lds = sizeof(unsigned) * (size_t)max_rows * (stage_pitch + kRsMidPitch);   // <= 80 * 136 * 4 = 43520 bytes
  hipLaunchKernelGGL(resize_u8_kernel, grid, block, lds, (hipStream_t)stream, src, dst, H, W, h, w, hbounds, hcoeffs, kx,
                     vbounds, vcoeffs, ky, max_rows, max_cols, stage_pitch);
  return (int)hipGetLastError();
}

}  // extern "C"
