// Transparency on the device (gfx950): straight-alpha RGBA images <-> the batch slots the RGB forward takes as they are.
// image_utils.rgba_split_f32 / rgba_merge_u8 are the definition; both kernels equal them bit for bit.
//
// split: uint8 [N][H][W][4] -> fp32 [N + K][3][H][W].  Slot n holds image n's colour planes; an image with
// alpha_slot[n] = s in [N, N + K) also fills slot s with its alpha plane three times (a grey image: the alpha goes through
// the same network as the colour).  merge: uint8 [N + K][h][w][3] (the forward's result) -> uint8 [N][h][w][4]: colour from
// slot n, alpha = (r + g + b + 1) / 3 of slot s in integers (the nearest integer to the mean), 255 for an image without a
// slot.  alpha_slot is a DEVICE table; an entry outside [N, N + K) means "opaque" -- no entry can send an access outside
// the tensors.
//
// Both kernels are pointwise and HBM-bound.  All layouts are contiguous over the H W pixels of an image, so the kernels walk
// pixels, not rows.  A = 16: a lane owns 4 consecutive pixels -- one 16-byte access to the RGBA image, one 16-byte store
// per fp32 plane (split), 12 + 12 bytes of the RGB images as 4-byte loads (merge); valid when H W is a multiple of 4 (every
// image and plane then starts on such a boundary) and the base pointers are aligned.  Otherwise one pixel per lane: the
// RGBA pixel as one 4-byte word where the image is 4-byte aligned (A = 4), else as bytes (A = 1).  The values do not
// depend on the path.  Flat grid over all pixels (groups) of the batch, counted in 64 bits, capped, grid-stride loop.
#include "larva_common.h"

namespace larva {

constexpr int kRgbaMaxBlocks = 2048;   // workgroups of a launch; beyond that the grid-stride loop takes over

__device__ __forceinline__ int alpha_slot_of(const int* __restrict__ alpha_slot, long long n, int N, int K) {
  const int s = alpha_slot[n];
  return (s >= N && s < N + K) ? s : -1;
}

template <int A>
__global__ __launch_bounds__(256) void rgba_u8_split_f32_kernel(const unsigned char* __restrict__ in,
                                                                const int* __restrict__ alpha_slot,
                                                                float* __restrict__ out, int N, int K, long long HW,
                                                                long long total) {
  // total: pixel quads (A == 16) or pixels of the N images
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    if constexpr (A == 16) {
      const long long per = HW >> 2, n = i / per, q = i - n * per;
      const int s = alpha_slot_of(alpha_slot, n, N, K);
      const u32x4 d = *reinterpret_cast<const u32x4*>(in + 16 * i);
      float* dst = out + n * 3 * HW + 4 * q;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<f32x4*>(dst + c * HW) =
            f32x4{(float)((d[0] >> (8 * c)) & 255u), (float)((d[1] >> (8 * c)) & 255u), (float)((d[2] >> (8 * c)) & 255u),
                  (float)((d[3] >> (8 * c)) & 255u)};
      if (s >= 0) {
        const f32x4 a = f32x4{(float)(d[0] >> 24), (float)(d[1] >> 24), (float)(d[2] >> 24), (float)(d[3] >> 24)};
        float* adst = out + (long long)s * 3 * HW + 4 * q;
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(adst + c * HW) = a;
      }
    } else {
      const long long n = i / HW, p = i - n * HW;
      const int s = alpha_slot_of(alpha_slot, n, N, K);
      unsigned d;
      if constexpr (A == 4) {
        d = *reinterpret_cast<const unsigned*>(in + 4 * i);
      } else {
        const unsigned char* src = in + 4 * i;
        d = src[0] | ((unsigned)src[1] << 8) | ((unsigned)src[2] << 16) | ((unsigned)src[3] << 24);
      }
      float* dst = out + n * 3 * HW + p;
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[c * HW] = (float)((d >> (8 * c)) & 255u);
      if (s >= 0) {
        const float a = (float)(d >> 24);
        float* adst = out + (long long)s * 3 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) adst[c * HW] = a;
      }
    }
  }
}

// the nearest integer to (r + g + b) / 3 (a third has no ties)
__device__ __forceinline__ unsigned mean3(unsigned r, unsigned g, unsigned b) { return (r + g + b + 1u) / 3u; }

template <int A>
__global__ __launch_bounds__(256) void rgb_u8_merge_rgba_kernel(const unsigned char* __restrict__ rgb,
                                                                const int* __restrict__ alpha_slot,
                                                                unsigned char* __restrict__ out, int N, int K, long long HW,
                                                                long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    if constexpr (A == 16) {
      const long long per = HW >> 2, n = i / per, q = i - n * per;
      const int s = alpha_slot_of(alpha_slot, n, N, K);
      const unsigned* src = reinterpret_cast<const unsigned*>(rgb + 12 * i);
      const unsigned c0 = src[0], c1 = src[1], c2 = src[2];
      unsigned a[4] = {255u, 255u, 255u, 255u};
      if (s >= 0) {
        const unsigned* asrc = reinterpret_cast<const unsigned*>(rgb + 3 * ((long long)s * HW + 4 * q));
        const unsigned a0 = asrc[0], a1 = asrc[1], a2 = asrc[2];
        a[0] = mean3(a0 & 255u, (a0 >> 8) & 255u, (a0 >> 16) & 255u);
        a[1] = mean3(a0 >> 24, a1 & 255u, (a1 >> 8) & 255u);
        a[2] = mean3((a1 >> 16) & 255u, a1 >> 24, a2 & 255u);
        a[3] = mean3((a2 >> 8) & 255u, (a2 >> 16) & 255u, a2 >> 24);
      }
      // the 12 colour bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 -> four words r g b a
      u32x4 o;
      o[0] = (c0 & 0x00ffffffu) | (a[0] << 24);
      o[1] = (c0 >> 24) | ((c1 & 0x0000ffffu) << 8) | (a[1] << 24);
      o[2] = (c1 >> 16) | ((c2 & 0x000000ffu) << 16) | (a[2] << 24);
      o[3] = (c2 >> 8) | (a[3] << 24);
      *reinterpret_cast<u32x4*>(out + 16 * i) = o;
    } else {
      const long long n = i / HW, p = i - n * HW;
      const int s = alpha_slot_of(alpha_slot, n, N, K);
      const unsigned char* src = rgb + 3 * i;
      const unsigned r = src[0], g = src[1], b = src[2];
      unsigned a = 255u;
      if (s >= 0) {
        const unsigned char* asrc = rgb + 3 * ((long long)s * HW + p);
        a = mean3(asrc[0], asrc[1], asrc[2]);
      }
      unsigned char* dst = out + 4 * i;
      if constexpr (A == 4) {
        *reinterpret_cast<unsigned*>(dst) = r | (g << 8) | (b << 16) | (a << 24);
      } else {
        dst[0] = (unsigned char)r, dst[1] = (unsigned char)g, dst[2] = (unsigned char)b, dst[3] = (unsigned char)a;
      }
    }
  }
}

static inline bool rgba_shape_ok(int N, int K, int H, int W) {
  return N > 0 && K >= 0 && K <= N && H > 0 && W > 0 && ((long long)N + K) * H * W * 3 < (1ll << 40);
}

static inline unsigned rgba_grid(long long total) {
  const long long g = (total + 255) / 256;
  return (unsigned)(g > kRgbaMaxBlocks ? kRgbaMaxBlocks : g);
}

static inline bool rgba_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace larva

using namespace larva;

extern "C" {

int larva_rgba_u8_split_f32(const unsigned char* rgba, const int* alpha_slot, float* out, int N, int K, int H, int W,
                            void* stream) {
  if (!rgba || !alpha_slot || !out || !rgba_shape_ok(N, K, H, W)) return (int)hipErrorInvalidValue;
  if (!rgba_aligned(out, 4) || !rgba_aligned(alpha_slot, 4)) return (int)hipErrorInvalidValue;
  const long long HW = (long long)H * W;
  const dim3 block(256);
  hipStream_t s = (hipStream_t)stream;
  if (HW % 4 == 0 && rgba_aligned(rgba, 16) && rgba_aligned(out, 16)) {
    const long long total = N * (HW / 4);
    hipLaunchKernelGGL(rgba_u8_split_f32_kernel<16>, dim3(rgba_grid(total)), block, 0, s, rgba, alpha_slot, out, N, K, HW, total);
  } else if (rgba_aligned(rgba, 4)) {
    const long long total = N * HW;
    hipLaunchKernelGGL(rgba_u8_split_f32_kernel<4>, dim3(rgba_grid(total)), block, 0, s, rgba, alpha_slot, out, N, K, HW, total);
  } else {
    const long long total = N * HW;
    hipLaunchKernelGGL(rgba_u8_split_f32_kernel<1>, dim3(rgba_grid(total)), block, 0, s, rgba, alpha_slot, out, N, K, HW, total);
  }
  return (int)hipGetLastError();
}

int larva_rgb_u8_merge_rgba(const unsigned char* rgb, const int* alpha_slot, unsigned char* out, int N, int K, int h, int w,
                            void* stream) {
  if (!rgb || !alpha_slot || !out || !rgba_shape_ok(N, K, h, w)) return (int)hipErrorInvalidValue;
  if (!rgba_aligned(alpha_slot, 4)) return (int)hipErrorInvalidValue;
  const long long HW = (long long)h * w;
  const dim3 block(256);
  hipStream_t s = (hipStream_t)stream;
  if (HW % 4 == 0 && rgba_aligned(rgb, 4) && rgba_aligned(out, 16)) {
    const long long total = N * (HW / 4);
    hipLaunchKernelGGL(rgb_u8_merge_rgba_kernel<16>, dim3(rgba_grid(total)), block, 0, s, rgb, alpha_slot, out, N, K, HW, total);
  } else if (rgba_aligned(out, 4)) {
    const long long total = N * HW;
    hipLaunchKernelGGL(rgb_u8_merge_rgba_kernel<4>, dim3(rgba_grid(total)), block, 0, s, rgb, alpha_slot, out, N, K, HW, total);
  } else {
    const long long total = N * HW;
    hipLaunchKernelGGL(rgb_u8_merge_rgba_kernel<1>, dim3(rgba_grid(total)), block, 0, s, rgb, alpha_slot, out, N, K, HW, total);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
