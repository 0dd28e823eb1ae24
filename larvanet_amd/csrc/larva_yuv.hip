// The video path's two colour conversions on the device (gfx950): planar YUV 4:2:0 frames (I420) -> the fp32 RGB planes
// the network reads, and the network's uint8 RGB image -> an I420 frame.  image_utils.i420_to_rgb_f32 / rgb_u8_to_i420 are
// the definition, in exact int32 arithmetic; both kernels equal them bit for bit, for all four matrix / range
// combinations: the coefficients arrive as a small int32 table built on the host (image_utils.yuv_to_rgb_table /
// rgb_to_yuv_table) and travel as a kernel argument, so one kernel per direction serves them all and a launch allocates
// and copies nothing.
//
// A frame is one buffer: Y [H][W], U [ch][cw], V [ch][cw], cw = (W + 1) / 2, ch = (H + 1) / 2; frame n of a batch starts at
// n * frame_pitch bytes.  Chroma is centred in its 2 x 2 luma block.  A coordinate outside a plane is clamped to the edge
// when reading, and nothing outside a plane is written.
//
// Both kernels are pointwise and HBM-bound.  A thread owns 2 luma rows x 4 luma columns = a 1 x 2 run of chroma samples:
// every chroma sample is read (to RGB: with its 3 x 4 neighbourhood) or made (from RGB) once for the pixels it serves, and
// a colour plane's four floats of a row go out as one 16-byte store.  Threads walk a frame's blocks row-major in a
// grid-stride loop over N * ceil(H / 2) * ceil(W / 4) blocks, counted in 64 bits.  Rows of W or 3 W bytes have no
// alignment of their own: the wide accesses are taken where W (and the pitch and the pointers) allow them, otherwise the
// same values move in narrower pieces; the results do not depend on the path.
#include "larva_common.h"

namespace larva {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kYuvMaxDim = 1 << 15;   // frame sides the launchers accept
constexpr int kYuvMaxBlocks = 2048;   // workgroups of a launch; beyond that the grid-stride loop takes over

struct YuvToRgbTable {
  int offset, cy, crv, cgu, cgv, cbu;   // luma offset; inverse-matrix entries * 4096
};
struct RgbToYuvTable {
  int offset, y[3], u[3], v[3];         // luma offset; forward-matrix rows * 65536
};

// clamp((n + 128) >> 8, 0, 255 * 256) / 256: 16 fractional bits -> 8, exact in fp32
__device__ __forceinline__ float rgb_value(int n) {
  return (float)min(max((n + 128) >> 8, 0), 255 * 256) * (1.0f / 256.0f);
}

// A: floats per store of an output row (4: W % 4 == 0 and out 16-byte aligned; 2: W % 2 == 0 and out 8-byte aligned; 1).
template <int A>
__global__ __launch_bounds__(256) void i420_to_rgb_f32_kernel(const unsigned char* __restrict__ frames, long long pitch,
                                                              float* __restrict__ out, int H, int W, long long total,
                                                              YuvToRgbTable t) {
  const int cw = (W + 1) >> 1, ch = (H + 1) >> 1, bw = (W + 3) >> 2;
  const long long per = (long long)ch * bw, HW = (long long)H * W;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long n = e / per;
    const int r = (int)(e - n * per), i = r / bw, b = r - i * bw;
    const unsigned char* yp = frames + n * pitch;
    const unsigned char* up = yp + HW;
    const unsigned char* vp = up + (long long)ch * cw;
    const int x0 = 4 * b;
    // the 3 x 4 chroma neighbourhood of the 1 x 2 chroma run (2 b, 2 b + 1), clamped
    const int rows[3] = {max(i - 1, 0), i, min(i + 1, ch - 1)};
    const int cols[4] = {max(2 * b - 1, 0), 2 * b, min(2 * b + 1, cw - 1), min(2 * b + 2, cw - 1)};
    int cu[3][4], cv[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long long at = (long long)rows[a] * cw + cols[c];
        cu[a][c] = up[at];
        cv[a][c] = vp[at];
      }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int y = 2 * i + a;
      if (y >= H) break;
      const unsigned char* yrow = yp + (long long)y * W;
      int lum[4];
      if constexpr (A == 4) {   // (W % 4 == 0: the whole run is inside the row; 4-byte aligned by the launcher's rule)
        const unsigned d = *reinterpret_cast<const unsigned*>(yrow + x0);
        lum[0] = d & 255u, lum[1] = (d >> 8) & 255u, lum[2] = (d >> 16) & 255u, lum[3] = d >> 24;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) lum[k] = yrow[min(x0 + k, W - 1)];
      }
      const int near = a ? 2 : 0;   // the nearer chroma row beside row 1
      f32x4 px[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = 1 + (k >> 1), nb = (k & 1) ? c + 1 : c - 1;
        const int u16 = 9 * cu[1][c] + 3 * cu[1][nb] + 3 * cu[near][c] + cu[near][nb] - 2048;
        const int v16 = 9 * cv[1][c] + 3 * cv[1][nb] + 3 * cv[near][c] + cv[near][nb] - 2048;
        const int l = (lum[k] - t.offset) * (16 * t.cy);
        px[0][k] = rgb_value(l + t.crv * v16);
        px[1][k] = rgb_value(l + t.cgu * u16 + t.cgv * v16);
        px[2][k] = rgb_value(l + t.cbu * u16);
      }
      float* dst = out + n * 3 * HW + (long long)y * W + x0;
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        float* d = dst + p * HW;
        if constexpr (A == 4) {
          *reinterpret_cast<f32x4*>(d) = px[p];
        } else if constexpr (A == 2) {   // (W even: pairs are inside the row or outside it)
          if (x0 < W) *reinterpret_cast<f32x2*>(d) = f32x2{px[p][0], px[p][1]};
          if (x0 + 2 < W) *reinterpret_cast<f32x2*>(d + 2) = f32x2{px[p][2], px[p][3]};
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (x0 + k < W) d[k] = px[p][k];
        }
      }
    }
  }
}

// clamp(n >> SHIFT, 0, 255), written as a clamp of n followed by a logical shift (the same value for every int n).  The
// shift-then-clamp form of two neighbouring bytes is selected as one v_ashr_pk_u8_i32 by hipcc (ROCm 7.2), and on
// gfx950 that instruction leaves bits 31:16 of its destination as they were while the compiler takes them for zero:
// OR-ing further bytes into the word (the 4-byte luma store below) then picked up stale bits in byte 2.
template <int SHIFT>
__device__ __forceinline__ unsigned shift_to_byte(int n) {
  return (unsigned)min(max(n, 0), (256 << SHIFT) - 1) >> SHIFT;
}
__device__ __forceinline__ unsigned luma_byte(const RgbToYuvTable& t, int r, int g, int b) {
  return shift_to_byte<16>(t.y[0] * r + t.y[1] * g + t.y[2] * b + (t.offset << 16) + (1 << 15));
}
__device__ __forceinline__ unsigned chroma_byte(const int c[3], int r, int g, int b) {
  return shift_to_byte<18>(c[0] * r + c[1] * g + c[2] * b + (128 << 18) + (1 << 17));
}

// VEC: W % 4 == 0, img 4-byte aligned, out and the pitch 4-byte aligned: a row's 12 bytes come as three 4-byte loads, the
// four luma bytes leave as one 4-byte store and the two bytes of a chroma plane as one 2-byte store.
template <bool VEC>
__global__ __launch_bounds__(256) void rgb_u8_to_i420_kernel(const unsigned char* __restrict__ img,
                                                             unsigned char* __restrict__ out, long long pitch, int H, int W,
                                                             long long total, RgbToYuvTable t) {
  const int cw = (W + 1) >> 1, ch = (H + 1) >> 1, bw = (W + 3) >> 2;
  const long long per = (long long)ch * bw, HW = (long long)H * W;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long n = e / per;
    const int r = (int)(e - n * per), i = r / bw, b = r - i * bw;
    const unsigned char* src = img + n * 3 * HW;
    unsigned char* yp = out + n * pitch;
    unsigned char* up = yp + HW;
    unsigned char* vp = up + (long long)ch * cw;
    const int x0 = 4 * b;
    int s[2][3] = {{0, 0, 0}, {0, 0, 0}};   // per-channel sums of the two 2 x 2 blocks
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int y = 2 * i + a, yr = min(y, H - 1);   // (row H of an odd-height image repeats row H - 1)
      const unsigned char* row = src + 3 * ((long long)yr * W);
      int q[12];
      if constexpr (VEC) {
        const unsigned* p = reinterpret_cast<const unsigned*>(row + 3 * x0);
        const unsigned d[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) q[k] = (d[k >> 2] >> (8 * (k & 3))) & 255u;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned char* p = row + 3 * (long long)min(x0 + k, W - 1);
          q[3 * k] = p[0], q[3 * k + 1] = p[1], q[3 * k + 2] = p[2];
        }
      }
      unsigned lum[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lum[k] = luma_byte(t, q[3 * k], q[3 * k + 1], q[3 * k + 2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[k >> 1][c] += q[3 * k + c];
      }
      if (y < H) {
        unsigned char* d = yp + (long long)y * W + x0;
        if constexpr (VEC) {
          *reinterpret_cast<unsigned*>(d) = lum[0] | (lum[1] << 8) | (lum[2] << 16) | (lum[3] << 24);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (x0 + k < W) d[k] = (unsigned char)lum[k];
        }
      }
    }
    const long long at = (long long)i * cw + 2 * b;
    const unsigned u0 = chroma_byte(t.u, s[0][0], s[0][1], s[0][2]), u1 = chroma_byte(t.u, s[1][0], s[1][1], s[1][2]);
    const unsigned v0 = chroma_byte(t.v, s[0][0], s[0][1], s[0][2]), v1 = chroma_byte(t.v, s[1][0], s[1][1], s[1][2]);
    if constexpr (VEC) {   // (cw even: both samples exist)
      *reinterpret_cast<unsigned short*>(up + at) = (unsigned short)(u0 | (u1 << 8));
      *reinterpret_cast<unsigned short*>(vp + at) = (unsigned short)(v0 | (v1 << 8));
    } else {
      if (2 * b < cw) up[at] = (unsigned char)u0, vp[at] = (unsigned char)v0;
      if (2 * b + 1 < cw) up[at + 1] = (unsigned char)u1, vp[at + 1] = (unsigned char)v1;
    }
  }
}

static inline long long yuv_frame_bytes(int H, int W) {
  return (long long)H * W + 2ll * ((H + 1) / 2) * ((W + 1) / 2);
}

static inline bool yuv_shape_ok(const void* a, const void* b, const void* table, long long pitch, int N, int H, int W) {
  return a && b && table && N >= 1 && H >= 1 && W >= 1 && H <= kYuvMaxDim && W <= kYuvMaxDim &&
         pitch >= yuv_frame_bytes(H, W);
}

static inline long long yuv_blocks(int N, int H, int W) { return (long long)N * ((H + 1) / 2) * ((W + 3) / 4); }

static inline unsigned yuv_grid(long long total) {
  const long long g = (total + 255) / 256;
  return (unsigned)(g > kYuvMaxBlocks ? kYuvMaxBlocks : g);
}

static inline bool aligned_to(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace larva

using namespace larva;

extern "C" {

int larva_i420_to_rgb_f32(const unsigned char* frames, long long frame_pitch_bytes, float* out, int N, int H, int W,
                          const int* coef_table, void* stream) {
  if (!yuv_shape_ok(frames, out, coef_table, frame_pitch_bytes, N, H, W)) return (int)hipErrorInvalidValue;
  const YuvToRgbTable t = {coef_table[0], coef_table[1], coef_table[2], coef_table[3], coef_table[4], coef_table[5]};
  // the int32 sums: |Y - offset| 16 cy <= 255 * 16 * 8192 and two chroma terms of at most 2048 * 16384 stay below 2^31
  if (t.offset < 0 || t.offset > 255 || t.cy < 0 || t.cy > 8192) return (int)hipErrorInvalidValue;
  for (int k = 2; k < 6; ++k)
    if (coef_table[k] < -16384 || coef_table[k] > 16384) return (int)hipErrorInvalidValue;
  const long long total = yuv_blocks(N, H, W);
  const dim3 grid(yuv_grid(total)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (W % 4 == 0 && frame_pitch_bytes % 4 == 0 && aligned_to(frames, 4) && aligned_to(out, 16))
    hipLaunchKernelGGL(i420_to_rgb_f32_kernel<4>, grid, block, 0, s, frames, frame_pitch_bytes, out, H, W, total, t);
  else if (W % 2 == 0 && aligned_to(out, 8))
    hipLaunchKernelGGL(i420_to_rgb_f32_kernel<2>, grid, block, 0, s, frames, frame_pitch_bytes, out, H, W, total, t);
  else
    hipLaunchKernelGGL(i420_to_rgb_f32_kernel<1>, grid, block, 0, s, frames, frame_pitch_bytes, out, H, W, total, t);
  return (int)hipGetLastError();
}

int larva_rgb_u8_to_i420(const unsigned char* img, unsigned char* out, long long frame_pitch_bytes, int N, int H, int W,
                         const int* coef_table, void* stream) {
  if (!yuv_shape_ok(img, out, coef_table, frame_pitch_bytes, N, H, W)) return (int)hipErrorInvalidValue;
  RgbToYuvTable t;
  t.offset = coef_table[0];
  if (t.offset < 0 || t.offset > 255) return (int)hipErrorInvalidValue;
  for (int r = 0; r < 3; ++r) {
    // a row's |c| sum to at most 2 * 65536: the luma sum stays below 255 * 2^17 + 2^24 and a chroma sum below
    // 1020 * 2^17 + 2^25, both inside int32
    long long mag = 0;
    for (int c = 0; c < 3; ++c) {
      const int v = coef_table[1 + 3 * r + c];
      (r == 0 ? t.y : r == 1 ? t.u : t.v)[c] = v;
      mag += v < 0 ? -(long long)v : v;
    }
    if (mag > 2 * 65536) return (int)hipErrorInvalidValue;
  }
  const long long total = yuv_blocks(N, H, W);
  const dim3 grid(yuv_grid(total)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (W % 4 == 0 && frame_pitch_bytes % 4 == 0 && aligned_to(img, 4) && aligned_to(out, 4))
    hipLaunchKernelGGL(rgb_u8_to_i420_kernel<true>, grid, block, 0, s, img, out, frame_pitch_bytes, H, W, total, t);
  else
    hipLaunchKernelGGL(rgb_u8_to_i420_kernel<false>, grid, block, 0, s, img, out, frame_pitch_bytes, H, W, total, t);
  return (int)hipGetLastError();
}

}  // extern "C"
