// The x2 / x3 ends of the network (gfx950): base image, PixelShuffle(s) of the last conv of a leg / the V2 tail, the
// L1 exits scored at scale s and the unshuffled gradients the leg's backward reads.  At s = 2 / 3 that conv has
// 3 s^2 = 12 / 27 outputs, run as a plain-epilogue 32-output conv on zero-padded weights (csrc/conv3x3_mfma.hip's
// 32-channel instantiation): its output y is [N][cpad][H][pitch], channels [3 s^2, cpad) hold the padding rows'
// bias (zero).  The kernels here map that layout to and from the [N][C][sH][sW] image:
//     out[n][c][s y + i][s x + j] = y[n][c s^2 + i s + j][y][x] (+ base)
// Every kernel works on one LR pixel per thread -- all s x s sub-pixels of its C colours -- and the gradient kernels
// write all cpad channels of that pixel, padding included (as zeros: the dgrad multiplies them by zero weight rows,
// and 0 * NaN would be NaN).  The x4 path (larva_pointwise.hip, conv3x3_mfma.hip's shuffle epilogues) is not
// touched.
#include <algorithm>

#include "larva_common.h"
#include "larva_bicubic.h"

namespace larva {

// ---------------------------------------------------------------------------------------------
// F.interpolate(x, scale_factor=S, mode, align_corners=False) for S = 2, 3.  The sub-pixel phases are constants:
// output j of an S-block sits at src = x + (2j + 1 - S) / 2S, i.e. x - 1/4, x + 1/4 at x2 and x - 1/3, x, x + 1/3 at
// x3, so every tap lies in the 5 x 5 window x - 2 .. x + 2 (index-clamped), loaded once per thread.  The phases are the
// exact ones (the C oracle's double-precision coordinates): ATen's float32 path computes src = (float)(1/3) * (dst +
// 0.5) - 0.5 at x3, whose rounding drifts along a row (up to ~1e-5 of a pixel on a DIV2K image), and that drift would
// make a band of rows interpolate differently from the same rows of the whole image.  Bicubic: taps floor(src) - 1 ..
// + 2, Keys A = -0.75, row pass first, then the column weights (ATen's separable order).  Bilinear: src clamped at 0,
// lambda = src - floor(src), the second tap clamped to the last index (upsample_bilinear2d).  One thread per LR pixel
// writes its S x S block.
// ---------------------------------------------------------------------------------------------
template <int N_>
__device__ __forceinline__ float pick(const float (&a)[N_], int k) {
  float r = a[0];
#pragma unroll
  for (int i = 1; i < N_; ++i) r = k == i ? a[i] : r;
  return r;
}

template <int S, int MODE>
__device__ __forceinline__ void axis_taps(int j, int lr, int& first, float (&w)[4]) {
  const int num = 2 * j + 1 - S;          // src - lr = num / 2S
  const int fl = num < 0 ? -1 : 0;        // floor(src) - lr
  const float t = (float)(num - 2 * S * fl) / (float)(2 * S);
  if constexpr (MODE == 0) {
    first = fl + 1;                        // window index of the first of 4 taps: 0 or 1
    cubic_coeffs(t, w);
  } else {
    const bool clamped = lr == 0 && fl < 0;   // src < 0: ATen clamps it to 0
    first = clamped ? 2 : fl + 2;          // window index of the first of 2 taps: 1 or 2
    w[1] = clamped ? 0.f : t;
    w[0] = 1.f - w[1];
    w[2] = w[3] = 0.f;
  }
}

template <int S, int MODE>   // MODE 0 bicubic, 1 bilinear
__global__ __launch_bounds__(256) void upsample_s_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         unsigned planes, unsigned H, unsigned W) {
  const unsigned total = planes * H * W;   // (< 2^31: checked by the launcher)
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned x = i % W, t2 = i / W, y = t2 % H, p = t2 / H;
  const float* src = in + (size_t)p * H * W;
  int col[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) col[c] = min(max((int)x - 2 + c, 0), (int)W - 1);
  float v[5][5];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const float* row = src + (size_t)min(max((int)y - 2 + r, 0), (int)H - 1) * W;
#pragma unroll
    for (int c = 0; c < 5; ++c) v[r][c] = row[col[c]];
  }
  int ox[S], oy[S];
  float wx[S][4], wy[S][4];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    axis_taps<S, MODE>(j, (int)x, ox[j], wx[j]);
    axis_taps<S, MODE>(j, (int)y, oy[j], wy[j]);
  }
  float* o = out + ((size_t)p * (S * H) + S * y) * (S * W) + S * x;
  constexpr int NT = MODE == 0 ? 4 : 2;   // taps per axis
  float h[S][5];   // row pass: output column phase jj, source row r
#pragma unroll
  for (int jj = 0; jj < S; ++jj)
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      float rowv;
      if constexpr (MODE == 0) {
        rowv = 0.f;
#pragma unroll
        for (int c = 0; c < NT; ++c) rowv += wx[jj][c] * pick(v[r], ox[jj] + c);
      } else {
        rowv = wx[jj][0] * pick(v[r], ox[jj]) + wx[jj][1] * pick(v[r], ox[jj] + 1);
      }
      h[jj][r] = rowv;
    }
#pragma unroll
  for (int ii = 0; ii < S; ++ii)
#pragma unroll
    for (int jj = 0; jj < S; ++jj) {
      float acc;
      if constexpr (MODE == 0) {
        acc = 0.f;
#pragma unroll
        for (int r = 0; r < NT; ++r) acc += wy[ii][r] * pick(h[jj], oy[ii] + r);
      } else {
        acc = wy[ii][0] * pick(h[jj], oy[ii]) + wy[ii][1] * pick(h[jj], oy[ii] + 1);
      }
      o[(size_t)ii * (S * W) + jj] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// out = PixelShuffle(S)(y[:, :C S^2]) (+ base): y [N][cpad][H][pitch] (columns [W, pitch) ignored), base / out
// [N][C][SH][SW].  One thread per LR pixel and colour.
// ---------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(256) void shuffle_base_kernel(const float* __restrict__ y, const float* __restrict__ base,
                                                           float* __restrict__ out, unsigned N, unsigned C, unsigned cpad,
                                                           unsigned H, unsigned W, unsigned P) {
  const unsigned total = N * C * H * W;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned x = i % W, t2 = i / W, yy = t2 % H, t3 = t2 / H, c = t3 % C, n = t3 / C;
  const size_t plane = (size_t)H * P;
  const float* src = y + ((size_t)n * cpad + c * S * S) * plane + (size_t)yy * P + x;
  const size_t o0 = (((size_t)n * C + c) * (S * H) + S * yy) * (S * W) + S * x;
#pragma unroll
  for (int ii = 0; ii < S; ++ii)
#pragma unroll
    for (int jj = 0; jj < S; ++jj) {
      const size_t o = o0 + (size_t)ii * (S * W) + jj;
      const float v = src[(ii * S + jj) * plane];
      out[o] = base ? v + base[o] : v;
    }
}

// ---------------------------------------------------------------------------------------------
// Unshuffled gradients, [N][cpad][H][W] with channels [C S^2, cpad) zero.  MODE 0: the inverse of PixelShuffle(S) of
// an HR gradient `a` (the backward of the tail's shuffle under a stand-alone L1 loss).  MODE 1: nn.L1Loss's backward
// at the exit, sign(a - b) * (gout[0] * gscale) / numel (sign(0) = 0, ATen's), straight in that layout.
// ---------------------------------------------------------------------------------------------
template <int S, int MODE>
__global__ __launch_bounds__(256) void unshuffle_s_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ gout, float gscale, float inv_numel,
                                                          float* __restrict__ out, unsigned N, unsigned C, unsigned cpad,
                                                          unsigned H, unsigned W) {
  const unsigned total = N * H * W;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned x = i % W, t2 = i / W, yy = t2 % H, n = t2 / H;
  const size_t plane = (size_t)H * W;
  float* o = out + (size_t)n * cpad * plane + (size_t)yy * W + x;
  float g = 0.f;
  if constexpr (MODE == 1) g = (gout[0] * gscale) * inv_numel;
  for (unsigned c = 0; c < C; ++c) {
    const size_t s0 = (((size_t)n * C + c) * (S * H) + S * yy) * (S * W) + S * x;
#pragma unroll
    for (int ii = 0; ii < S; ++ii)
#pragma unroll
      for (int jj = 0; jj < S; ++jj) {
        const size_t s = s0 + (size_t)ii * (S * W) + jj;
        float v;
        if constexpr (MODE == 0) {
          v = a[s];
        } else {
          const float d = a[s] - b[s];
          v = d > 0.f ? g : (d < 0.f ? -g : 0.f);
        }
        o[(c * S * S + ii * S + jj) * plane] = v;
      }
  }
  for (unsigned k = C * S * S; k < cpad; ++k) o[k * plane] = 0.f;
}

// ---------------------------------------------------------------------------------------------
// One training exit at scale S after its plain-epilogue conv, in one pass: o = PixelShuffle(S)(y) + base (stored only
// when `out` is given), block partial sums of |o - truth| (consumed by larva_loss_from_partials like
// larva_l1_partial's) and the gradient sign(o - truth) * g in the unshuffled [N][cpad][H][W] layout, padding channels
// zero.  The HR image is never written only to be read back.  y, grad: [N][cpad][H][W] (no row pitch).  Grid: a fixed
// number of blocks walking the LR pixels with a grid stride, so the partial sums do not depend on the launch.
// ---------------------------------------------------------------------------------------------
constexpr int kScaleL1Blocks = 1024;   // = larva_l1_workspace_floats()

template <int S>
__global__ __launch_bounds__(256) void shuffle_l1_grad_kernel(const float* __restrict__ y, const float* __restrict__ base,
                                                              const float* __restrict__ truth, float g,
                                                              float* __restrict__ partial, float* __restrict__ grad,
                                                              float* __restrict__ out, unsigned N, unsigned C,
                                                              unsigned cpad, unsigned H, unsigned W) {
  const unsigned total = N * H * W;
  const size_t plane = (size_t)H * W;
  float s = 0.f;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned x = i % W, t2 = i / W, yy = t2 % H, n = t2 / H;
    const size_t lr = (size_t)n * cpad * plane + (size_t)yy * W + x;
    for (unsigned c = 0; c < C; ++c) {
      const size_t h0 = (((size_t)n * C + c) * (S * H) + S * yy) * (S * W) + S * x;
#pragma unroll
      for (int ii = 0; ii < S; ++ii)
#pragma unroll
        for (int jj = 0; jj < S; ++jj) {
          const size_t h = h0 + (size_t)ii * (S * W) + jj;
          const size_t k = lr + (c * S * S + ii * S + jj) * plane;
          const float v = y[k] + base[h];
          const float d = v - truth[h];
          s += fabsf(d);
          grad[k] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
          if (out) out[h] = v;
        }
    }
    for (unsigned k = C * S * S; k < cpad; ++k) grad[lr + k * plane] = 0.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

static inline unsigned blocks_for(long long work) { return (unsigned)((work + 255) / 256); }

}  // namespace larva

using namespace larva;

extern "C" int larva_upsample4_fwd(const float* in, float* out, int N, int C, int H, int W, int mode, void* stream);

extern "C" {

// F.interpolate(x, scale_factor=scale, mode, align_corners=False), mode 0 bicubic / 1 bilinear, scale 2, 3 or 4
// (4 = larva_upsample4_fwd).  in [N][C][H][W] -> out [N][C][scale H][scale W].
int larva_upsample_fwd(const float* in, float* out, int N, int C, int H, int W, int scale, int mode, void* stream) {
  if (scale == 4) return larva_upsample4_fwd(in, out, N, C, H, W, mode, stream);
  if (!in || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1) || (scale != 2 && scale != 3))
    return (int)hipErrorInvalidValue;
  const long long px = (long long)N * C * H * W;
  if (px * scale * scale >= (1ll << 31) - 256) return (int)hipErrorInvalidValue;
  const dim3 grid(blocks_for(px)), block(256);
  hipStream_t s = (hipStream_t)stream;
  const unsigned planes = (unsigned)(N * C);
  if (scale == 2 && mode == 0) hipLaunchKernelGGL((upsample_s_kernel<2, 0>), grid, block, 0, s, in, out, planes, H, W);
  else if (scale == 2) hipLaunchKernelGGL((upsample_s_kernel<2, 1>), grid, block, 0, s, in, out, planes, H, W);
  else if (mode == 0) hipLaunchKernelGGL((upsample_s_kernel<3, 0>), grid, block, 0, s, in, out, planes, H, W);
  else hipLaunchKernelGGL((upsample_s_kernel<3, 1>), grid, block, 0, s, in, out, planes, H, W);
  return (int)hipGetLastError();
}

static int scale_shape_ok(int N, int C, int cpad, int H, int W, int scale) {
  return N > 0 && C > 0 && H > 0 && W > 0 && (scale == 2 || scale == 3) && cpad >= C * scale * scale &&
         (long long)N * cpad * H * W < (1ll << 31) - 256 && (long long)N * C * H * W * scale * scale < (1ll << 31) - 256;
}

// out [N][C][scale H][scale W] = PixelShuffle(scale)(y[:, :C scale^2]) + base (base may be NULL): y [N][cpad][H][pitch].
int larva_pixel_shuffle_base(const float* y, const float* base, float* out, int N, int C, int cpad, int H, int W,
                             int pitch, int scale, void* stream) {
  if (pitch == 0) pitch = W;
  if (!y || !out || pitch < W || !scale_shape_ok(N, C, cpad, H, pitch, scale)) return (int)hipErrorInvalidValue;
  const dim3 grid(blocks_for((long long)N * C * H * W)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (scale == 2)
    hipLaunchKernelGGL((shuffle_base_kernel<2>), grid, block, 0, s, y, base, out, N, C, cpad, H, W, pitch);
  else
    hipLaunchKernelGGL((shuffle_base_kernel<3>), grid, block, 0, s, y, base, out, N, C, cpad, H, W, pitch);
  return (int)hipGetLastError();
}

// in [N][C][scale H][scale W] -> out [N][cpad][H][W]: the inverse of PixelShuffle(scale), channels [C scale^2, cpad) zero.
int larva_pixel_unshuffle(const float* in, float* out, int N, int C, int cpad, int H, int W, int scale, void* stream) {
  if (!in || !out || !scale_shape_ok(N, C, cpad, H, W, scale)) return (int)hipErrorInvalidValue;
  const dim3 grid(blocks_for((long long)N * H * W)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (scale == 2)
    hipLaunchKernelGGL((unshuffle_s_kernel<2, 0>), grid, block, 0, s, in, nullptr, nullptr, 1.f, 1.f, out, N, C, cpad, H, W);
  else
    hipLaunchKernelGGL((unshuffle_s_kernel<3, 0>), grid, block, 0, s, in, nullptr, nullptr, 1.f, 1.f, out, N, C, cpad, H, W);
  return (int)hipGetLastError();
}

// nn.L1Loss backward in the unshuffled layout: a, b [N][C][scale H][scale W] -> ga [N][cpad][H][W],
// ga = sign(a - b) * (gout[0] * gscale) / numel, channels [C scale^2, cpad) zero.
int larva_l1_bwd_unshuffle(const float* a, const float* b, const float* gout, float gscale, float* ga, int N, int C,
                           int cpad, int H, int W, int scale, void* stream) {
  if (!a || !b || !gout || !ga || !scale_shape_ok(N, C, cpad, H, W, scale)) return (int)hipErrorInvalidValue;
  const float inv = 1.0f / (float)((long long)N * C * H * W * scale * scale);
  const dim3 grid(blocks_for((long long)N * H * W)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (scale == 2)
    hipLaunchKernelGGL((unshuffle_s_kernel<2, 1>), grid, block, 0, s, a, b, gout, gscale, inv, ga, N, C, cpad, H, W);
  else
    hipLaunchKernelGGL((unshuffle_s_kernel<3, 1>), grid, block, 0, s, a, b, gout, gscale, inv, ga, N, C, cpad, H, W);
  return (int)hipGetLastError();
}

// One training exit at scale 2 / 3 after its plain conv: out = PixelShuffle(scale)(y) + base (out may be NULL: not
// stored), `partial` receives *blocks_out <= larva_l1_workspace_floats() block partial sums of sum|out - truth|,
// grad [N][cpad][H][W] = sign(out - truth) * gvalue * gscale / numel (padding channels zero).  y [N][cpad][H][W].
int larva_shuffle_l1_partial_grad(const float* y, const float* base, const float* truth, float gvalue, float gscale,
                                  float* partial, int* blocks_out, float* grad, float* out, int N, int C, int cpad, int H,
                                  int W, int scale, void* stream) {
  if (!y || !base || !truth || !partial || !blocks_out || !grad || !scale_shape_ok(N, C, cpad, H, W, scale))
    return (int)hipErrorInvalidValue;
  const long long px = (long long)N * H * W;
  const unsigned blocks = (unsigned)std::min<long long>(kScaleL1Blocks, (long long)blocks_for(px));
  *blocks_out = (int)blocks;
  const float g = (gvalue * gscale) * (1.0f / (float)((long long)N * C * H * W * scale * scale));
  hipStream_t s = (hipStream_t)stream;
  if (scale == 2)
    hipLaunchKernelGGL((shuffle_l1_grad_kernel<2>), dim3(blocks), dim3(256), 0, s, y, base, truth, g, partial, grad, out,
                       N, C, cpad, H, W);
  else
    hipLaunchKernelGGL((shuffle_l1_grad_kernel<3>), dim3(blocks), dim3(256), 0, s, y, base, truth, g, partial, grad, out,
                       N, C, cpad, H, W);
  return (int)hipGetLastError();
}

}  // extern "C"
