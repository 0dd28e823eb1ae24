// Antialiased bicubic decimation of uint8 images by an integer scale s = 2, 3, 4 (gfx950): the forward direction of
// the degradation SR data is made with (the MATLAB imresize convention), exact in integers.
//
// Definition (image_utils.bicubic_downscale_u8 is the host restatement).  Input I [H][W] pixels, output h = H / s, w =
// W / s (floor); only the top-left h s x w s pixels are read.  Along one axis output i takes input j = s i + o, o =
// LO .. LO + NT - 1, with the integer weight T[o - LO] over D (Keys cubic, a = -1/2, stretched by s: the weights do not
// depend on i and sum to D); j outside [0, n) reflects, m = j mod 2 n, j' = m < n ? m : 2 n - 1 - m, n the CROPPED
// length.  out = clip(round_half_even(N / D^2), 0, 255) with N the exact integer double sum: one rounding, at the end.
//
// Kernel.  A 256-thread workgroup owns 8 rows x 96 output BYTES (32 RGB pixels of an interleaved image, C = 3; 96
// pixels of one colour plane, C = 1) and goes through LDS twice:
//   1. stage the IN_H x NB input bytes of the tile (IN_H = 8 s + NT - s rows, NB = (96 / C s + NT - s) C bytes) as
//      rows of PD dwords.  A tile whose columns need no reflection loads ALIGNED dwords: row r starts at the 4-byte
//      boundary at or below its first byte and keeps that byte's offset (skew_r = address & 3) -- a row of 3 W bytes has
//      no alignment of its own.  A load never touches a dword that holds no wanted byte.  Tiles at the left / right edge
//      go byte by byte with the reflected column (skew 0).  Rows reflect in both forms.
//   2. horizontal pass: a work item = (input row r, group g of 12 output bytes: 4 RGB pixels or 12 plane pixels).  Its
//      bytes start at dword 3 s g of the row: it reads ND + 1 dwords, shifts the skew out (v_alignbyte) and has every
//      tap at a compile-time position.  12 int32 sums (|v| <= 255 * 4800) go to mid[r][12 g ..], pitch 97.
//   3. vertical pass + rounding: thread -> (output row, output byte e), NT taps down mid in 64-bit integers (x4: |N| up
//      to 5.9e9), one floor division (a shift for D^2 = 2^16, 2^24; by 6561 at x3, where |N| < 2^31), half to even,
//      clip, one byte store; a wave stores contiguous runs of a row.
// LDS banks (ds_read_b32 / ds_write_b32: bank = dword address mod 32, per 32-lane half).  Staging: consecutive lanes,
// consecutive dwords.  Horizontal pass: the 32 lanes of a half are 32 consecutive ROWS of one group (items are [g][row
// slot], slots = 32 or 64): dword r PD + const and r 97 + const, PD and 97 odd -> 32 distinct banks on the read and on
// the write side.  Vertical pass: 96 = 3 x 32, a half-wave lies in one output row: 32 consecutive dwords.  No conflicts.
// No scratch, no atomics, nothing but the output is stored.
#include "larva_common.h"

namespace larva {

template <int S> struct DownTaps;
template <> struct DownTaps<2> {
  static constexpr int N = 8, LO = -3, SHIFT = 16;
  static constexpr int w[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
};
template <> struct DownTaps<3> {
  static constexpr int N = 11, LO = -4, SHIFT = 0;   // D^2 = 6561
  static constexpr int w[11] = {-1, -2, 0, 9, 21, 27, 21, 9, 0, -2, -1};
};
template <> struct DownTaps<4> {
  static constexpr int N = 16, LO = -6, SHIFT = 24;
  static constexpr int w[16] = {-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7};
};

constexpr int kDownRows = 8;     // output rows of a tile
constexpr int kDownBytes = 96;   // output bytes of a tile row (kernels.DOWN_TILE_ROWS / DOWN_TILE_BYTES mirror these)
constexpr int kDownMidPitch = 97;

// Symmetric reflection of any j into [0, n), n >= 1 (the edge is not repeated twice: -1 -> 0, n -> n - 1).
__device__ __forceinline__ int down_reflect(int j, int n) {
  if ((unsigned)j >= (unsigned)n) {
    if (j >= -n && j < 2 * n) {
      j = j < 0 ? -1 - j : 2 * n - 1 - j;
    } else {   // (short axes: the taps wrap more than once)
      int m = j % (2 * n);
      if (m < 0) m += 2 * n;
      j = m < n ? m : 2 * n - 1 - m;
    }
  }
  return j;
}

// clip(round_half_even(n / D^2), 0, 255)
template <int S>
__device__ __forceinline__ unsigned down_round(long long n) {
  long long q;
  if constexpr (DownTaps<S>::SHIFT != 0) {
    constexpr int sh = DownTaps<S>::SHIFT;
    constexpr long long half = 1ll << (sh - 1);
    q = n >> sh;                                  // floor, also for n < 0
    const long long rem = n & ((1ll << sh) - 1);  // n - q 2^sh in [0, 2^sh)
    if (rem > half || (rem == half && (q & 1))) ++q;
  } else {
    const int v = (int)n;   // |n| <= 255 * 93^2
    int qq = v / 6561, rem = v - qq * 6561;
    if (rem < 0) { --qq; rem += 6561; }
    if (2 * rem > 6561) ++qq;   // (6561 is odd: no tie)
    q = qq;
  }
  return (unsigned)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

// One tile (ty, tx) of one image: src = pixel (0, 0), `pitch` bytes per row, C interleaved channels; dst [h][w][C].
template <int S, int C>
__device__ __forceinline__ void down_tile(const unsigned char* __restrict__ src, long long pitch, int h, int w,
                                          unsigned char* __restrict__ dst, int ty, int tx) {
  using T = DownTaps<S>;
  constexpr int NT = T::N, LO = T::LO;
  constexpr int R = 12 / C, TW = kDownBytes / C, TH = kDownRows, MP = kDownMidPitch;
  constexpr int IN_H = TH * S + NT - S, IN_W = TW * S + NT - S, NB = IN_W * C;
  constexpr int ND = (((R - 1) * S + NT) * C + 3) / 4;   // dwords that hold an item's bytes
  constexpr int DPR = (NB + 3 + 3) / 4;                  // dwords of a staged row, any skew
  constexpr int PD0 = DPR > 3 * S * 7 + ND + 1 ? DPR : 3 * S * 7 + ND + 1;
  constexpr int PD = PD0 | 1;
  constexpr int SLOTS = IN_H <= 32 ? 32 : 64;
  static_assert(C == 1 || C == 3, "channels");
  __shared__ unsigned in_t[IN_H * PD];
  __shared__ int mid[IN_H * MP];

  const int tid = threadIdx.x;
  const int Hc = h * S, Wc = w * S;
  const int r_start = S * TH * ty + LO, c_start = S * TW * tx + LO;
  const bool fast = c_start >= 0 && c_start + IN_W <= Wc;   // (uniform: no column of the tile reflects)
  const unsigned char* col0 = src + (long long)c_start * C;

  if (fast) {
    // (every load of the thread is issued before the first LDS store: one memory latency per tile, not one per dword)
    constexpr int LOADS = (IN_H * DPR + 255) / 256;
    unsigned held[LOADS];
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
      const int e = tid + 256 * k, r = e / DPR, d = e - r * DPR;
      held[k] = 0;
      if (e < IN_H * DPR) {
        const unsigned char* p = col0 + (long long)down_reflect(r_start + r, Hc) * pitch;
        const int skew = (int)(reinterpret_cast<uintptr_t>(p) & 3);
        if (4 * d < skew + NB) held[k] = *reinterpret_cast<const unsigned*>(p - skew + 4 * d);
      }
    }
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
      const int e = tid + 256 * k, r = e / DPR, d = e - r * DPR;
      if (e < IN_H * DPR) in_t[r * PD + d] = held[k];
    }
  } else {
    unsigned char* in_b = reinterpret_cast<unsigned char*>(in_t);
    for (int e = tid; e < IN_H * NB; e += 256) {
      const int r = e / NB, b = e - r * NB, col = b / C, ch = b - col * C;
      in_b[r * (PD * 4) + b] = src[(long long)down_reflect(r_start + r, Hc) * pitch +
                                   (long long)down_reflect(c_start + col, Wc) * C + ch];
    }
  }
  __syncthreads();

  for (int it = tid; it < 8 * SLOTS; it += 256) {
    const int g = it / SLOTS, r = it - g * SLOTS;
    if (r < IN_H) {
      unsigned skew = 0;
      if (fast)
        skew = (unsigned)(reinterpret_cast<uintptr_t>(col0 + (long long)down_reflect(r_start + r, Hc) * pitch) & 3);
      unsigned raw[ND + 1], by[ND];
#pragma unroll
      for (int i = 0; i <= ND; ++i) raw[i] = in_t[r * PD + 3 * S * g + i];
#pragma unroll
      for (int i = 0; i < ND; ++i) by[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], skew);
#pragma unroll
      for (int p = 0; p < R; ++p) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          int acc = 0;
#pragma unroll
          for (int k = 0; k < NT; ++k) {
            const int j = (p * S + k) * C + c;
            acc += T::w[k] * (int)((by[j >> 2] >> (8 * (j & 3))) & 255u);
          }
          mid[r * MP + 12 * g + p * C + c] = acc;
        }
      }
    }
  }
  __syncthreads();

  for (int idx = tid; idx < TH * kDownBytes; idx += 256) {
    const int oy = idx / kDownBytes, e = idx - oy * kDownBytes;
    long long n = 0;
#pragma unroll
    for (int k = 0; k < NT; ++k) n += (long long)T::w[k] * mid[(S * oy + k) * MP + e];
    const int y = TH * ty + oy, x = TW * tx + e / C;
    if (y < h && x < w) dst[((long long)y * w + (long long)TW * tx) * C + e] = (unsigned char)down_round<S>(n);
  }
}

template <int S>
__global__ __launch_bounds__(256) void bicubic_down_kernel(const unsigned char* __restrict__ src, long long pitch, int h,
                                                           int w, unsigned char* __restrict__ dst) {
  down_tile<S, 3>(src, pitch, h, w, dst, blockIdx.y, blockIdx.x);
}

// Flat grid over (image, plane, tile): prefix[i] = tiles of the images before i (prefix[n] = the grid); a workgroup
// finds its image by bisection.  C = 3: interleaved HWC images; C = 1: CHW images, three planes each.
template <int S, int C>
__global__ __launch_bounds__(256) void bicubic_down_table_kernel(const unsigned char* __restrict__ data,
                                                                 const long long* __restrict__ offsets,
                                                                 const int* __restrict__ hw, unsigned char* __restrict__ out,
                                                                 const long long* __restrict__ out_offsets,
                                                                 const int* __restrict__ prefix, int n) {
  const int b = blockIdx.x;
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (prefix[m] <= b) lo = m; else hi = m;
  }
  const int H = hw[2 * lo], W = hw[2 * lo + 1], h = H / S, w = W / S;
  if (h < 1 || w < 1) return;
  constexpr int TW = kDownBytes / C;
  const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + kDownRows - 1) / kDownRows;
  const int local = b - prefix[lo], per_plane = tiles_x * tiles_y;
  const int plane = local / per_plane, t = local - plane * per_plane;
  if (local < 0 || plane >= (C == 1 ? 3 : 1)) return;   // (a prefix table that disagrees with the shapes)
  const unsigned char* src = data + offsets[lo] + (long long)plane * H * W;
  unsigned char* dst = out + out_offsets[lo] + (long long)plane * h * w;
  down_tile<S, C>(src, (long long)W * C, h, w, dst, t / tiles_x, t - (t / tiles_x) * tiles_x);
}

}  // namespace larva

using namespace larva;

extern "C" {

// dst uint8 [H / s][W / s][3] = the bicubic decimation by s = 2, 3, 4 of src uint8 [H][W][3] with `pitch` bytes per row.
int larva_bicubic_down_u8(const unsigned char* src, int H, int W, long long pitch, int s, unsigned char* dst,
                          void* stream) {
  if (!src || !dst || s < 2 || s > 4 || H < s || W < s || H > (1 << 20) || W > (1 << 20) || pitch < 3ll * W)
    return (int)hipErrorInvalidValue;
  const int h = H / s, w = W / s;
  constexpr int TW = kDownBytes / 3;
  const dim3 grid((w + TW - 1) / TW, (h + kDownRows - 1) / kDownRows), block(256);
  if (grid.y > 65535u) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (s == 2) hipLaunchKernelGGL(bicubic_down_kernel<2>, grid, block, 0, st, src, pitch, h, w, dst);
  else if (s == 3) hipLaunchKernelGGL(bicubic_down_kernel<3>, grid, block, 0, st, src, pitch, h, w, dst);
  else hipLaunchKernelGGL(bicubic_down_kernel<4>, grid, block, 0, st, src, pitch, h, w, dst);
  return (int)hipGetLastError();
}

// The dataset form: every image of a byte table in one launch (see include/larva_hip.h).
int larva_bicubic_down_u8_table(const unsigned char* data, const long long* offsets, const int* hw, int n, int s,
                                int planar, unsigned char* out, const long long* out_offsets, const int* tile_prefix,
                                int total_tiles, void* stream) {
  if (!data || !offsets || !hw || !out || !out_offsets || !tile_prefix || n < 1 || s < 2 || s > 4 || total_tiles < 1)
    return (int)hipErrorInvalidValue;
  const dim3 grid(total_tiles), block(256);
  hipStream_t st = (hipStream_t)stream;
#define LARVA_DOWN_TABLE(S, C) \
  hipLaunchKernelGGL((bicubic_down_table_kernel<S, C>), grid, block, 0, st, data, offsets, hw, out, out_offsets, tile_prefix, n)
  if (planar) {
    if (s == 2) LARVA_DOWN_TABLE(2, 1); else if (s == 3) LARVA_DOWN_TABLE(3, 1); else LARVA_DOWN_TABLE(4, 1);
  } else {
    if (s == 2) LARVA_DOWN_TABLE(2, 3); else if (s == 3) LARVA_DOWN_TABLE(3, 3); else LARVA_DOWN_TABLE(4, 3);
  }
#undef LARVA_DOWN_TABLE
  return (int)hipGetLastError();
}

}  // extern "C"
