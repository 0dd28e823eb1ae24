// Benchmark metrics of two uint8 HWC images on the device (gfx950): the exact sum of squared differences (PSNR) and the
// Gaussian-window SSIM of Wang et al. (11 taps, sigma 1.5, K1 0.01, K2 0.03, data range 255, population covariance), over
// a window (y0, x0, h, w) of both images, on the three colour planes or on the BT.601 luma plane.
//
// One launch, one workgroup (256 threads = 4 wave64) per output tile and plane:
//   * stage the tile + 5 pixels of halo of both images from their bytes into LDS as floats (exact integers), walking
//     pixels: a row's 3 w bytes need no alignment and the window may start anywhere.  In luma mode the conversion happens
//     here, so no Y plane is ever stored.  The squared error of the pixels this workgroup OWNS (every window pixel has
//     exactly one owner) is summed in integers on the way.
//   * row pass: the 11-tap sums of x, y, x^2, y^2, x y for kMetSY staged rows x kMetTX columns, in double, into LDS;
//   * column pass: the 11-tap sums over those, S per sample, summed per thread in a fixed order.
// Neither the moment maps nor the S map reach memory.  The filtered samples are the "valid" ones -- the window minus 5
// pixels on every side -- so no boundary rule of the filter is ever used.
//
// Everything that is summed across threads goes wave shuffle -> LDS -> one partial per workgroup in the workspace, and a
// second one-workgroup launch adds the partials in a fixed order: the result is bitwise reproducible and does not depend
// on what else is resident.  The moment sums are double (pixel values and their products are exact integers, so the
// variance's cancellation costs ~1e-11 of 65025): the same sums in float64 numpy agree with scipy's filter to 1e-15 in SSIM.
// The S expression is compiled without FMA contraction so that numerator and denominator are the same roundings when
// both images are equal: S is then exactly 1 (IEEE division), and so is the mean.
#include <algorithm>
#include <cmath>

#include "larva_common.h"

namespace larva {

constexpr int kMetR = 5;                       // filter radius: int(3.5 * 1.5 + 0.5)
constexpr int kMetTaps = 2 * kMetR + 1;
constexpr int kMetTX = 32, kMetTY = 22;        // SSIM samples per tile
constexpr int kMetSX = kMetTX + 2 * kMetR;     // staged columns (42)
constexpr int kMetSY = kMetTY + 2 * kMetR;     // staged rows (32)
constexpr int kMetPitch = kMetSX + 1;          // LDS row stride of a staged row (floats)
constexpr int kMetMaxDim = 1 << 15;            // window sides the launcher accepts

struct GaussTaps {
  double w[kMetTaps];
};

// BT.601 luma of an 8-bit triple, 16..235: 16 + round_half_even((65481 R + 128553 G + 24966 B) / 255000), in integers.
__device__ __forceinline__ int luma601(unsigned r, unsigned g, unsigned b) {
  const unsigned n = 65481u * r + 128553u * g + 24966u * b;   // <= 55 845 000
  unsigned q = n / 255000u;
  const unsigned rem2 = 2u * (n - q * 255000u);
  q += (rem2 > 255000u || (rem2 == 255000u && (q & 1u))) ? 1u : 0u;
  return 16 + (int)q;
}

__device__ __forceinline__ double ssim_sample(double ux, double uy, double uxx, double uyy, double uxy) {
#pragma clang fp contract(off)
  const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double vx = uxx - ux * ux, vy = uyy - uy * uy, vxy = uxy - ux * uy;
  const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
  const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
  return (a1 * a2) / (b1 * b2);
}

// MODE 0: colour plane blockIdx.z of three; MODE 1: the luma plane.  ssim == 0: squared error only, tiles of the whole
// staged size without overlap.  Partials: part_ssim[b], part_sse[b], b = (z gridDim.y + y) gridDim.x + x.
template <int MODE>
__global__ __launch_bounds__(256) void u8_metrics_kernel(const unsigned char* __restrict__ out, long long opitch,
                                                         const unsigned char* __restrict__ truth, long long tpitch,
                                                         int y0, int x0, int h, int w, int ssim, GaussTaps taps,
                                                         double* __restrict__ part_ssim,
                                                         unsigned long long* __restrict__ part_sse) {
  __shared__ float sa[kMetSY][kMetPitch], sb[kMetSY][kMetPitch];
  __shared__ double hb[5][kMetSY][kMetTX];
  __shared__ double wave_ssim[4];
  __shared__ unsigned long long wave_sse[4];
  const int tid = threadIdx.x, plane = blockIdx.z;
  const int r0 = blockIdx.y * (ssim ? kMetTY : kMetSY), c0 = blockIdx.x * (ssim ? kMetTX : kMetSX);   // window coordinates
  // the window pixels whose squared error this workgroup adds: with overlapping tiles, the tile's own centre region,
  // stretched to the window's edge by the first and the last tile of a row / column
  int own_r0 = r0, own_r1 = min(h, r0 + kMetSY), own_c0 = c0, own_c1 = min(w, c0 + kMetSX);
  if (ssim) {
    own_r0 = blockIdx.y == 0 ? 0 : r0 + kMetR;
    own_r1 = blockIdx.y == gridDim.y - 1 ? h : r0 + kMetR + kMetTY;
    own_c0 = blockIdx.x == 0 ? 0 : c0 + kMetR;
    own_c1 = blockIdx.x == gridDim.x - 1 ? w : c0 + kMetR + kMetTX;
  }
  unsigned sse = 0;   // (at most 6 pixels per thread)
  for (int e = tid; e < kMetSY * kMetSX; e += 256) {
    const int r = e / kMetSX, c = e - r * kMetSX;
    const int wr = r0 + r, wc = c0 + c;
    float a = 0.f, b = 0.f;
    if (wr < h && wc < w) {
      const unsigned char* po = out + (size_t)(y0 + wr) * opitch + 3 * (size_t)(x0 + wc);
      const unsigned char* pt = truth + (size_t)(y0 + wr) * tpitch + 3 * (size_t)(x0 + wc);
      int va, vb;
      if constexpr (MODE == 1) {
        va = luma601(po[0], po[1], po[2]);
        vb = luma601(pt[0], pt[1], pt[2]);
      } else {
        va = po[plane];
        vb = pt[plane];
      }
      const int d = va - vb;
      if (wr >= own_r0 && wr < own_r1 && wc >= own_c0 && wc < own_c1) sse += (unsigned)(d * d);
      a = (float)va;
      b = (float)vb;
    }
    sa[r][c] = a;
    sb[r][c] = b;
  }
  __syncthreads();
  double s = 0.0;
  if (ssim) {
    for (int e = tid; e < kMetSY * kMetTX; e += 256) {   // row pass: lanes walk a row, conflict-free
      const int r = e / kMetTX, c = e - r * kMetTX;
      double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
      for (int k = 0; k < kMetTaps; ++k) {
        const double x = (double)sa[r][c + k], y = (double)sb[r][c + k];
        const double wx = taps.w[k] * x, wy = taps.w[k] * y;
        mx += wx;
        my += wy;
        mxx = fma(wx, x, mxx);
        mxy = fma(wx, y, mxy);
        myy = fma(wy, y, myy);
      }
      hb[0][r][c] = mx;
      hb[1][r][c] = my;
      hb[2][r][c] = mxx;
      hb[3][r][c] = myy;
      hb[4][r][c] = mxy;
    }
    __syncthreads();
    for (int e = tid; e < kMetTY * kMetTX; e += 256) {   // column pass + S
      const int i = e / kMetTX, j = e - i * kMetTX;
      if (r0 + i < h - 2 * kMetR && c0 + j < w - 2 * kMetR) {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kMetTaps; ++k)
#pragma unroll
          for (int q = 0; q < 5; ++q) m[q] = fma(taps.w[k], hb[q][i + k][j], m[q]);
        s += ssim_sample(m[0], m[1], m[2], m[3], m[4]);
      }
    }
  }
  unsigned long long sse64 = sse;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    sse64 += __shfl_xor(sse64, o);
  }
  if ((tid & 63) == 0) {
    wave_ssim[tid >> 6] = s;
    wave_sse[tid >> 6] = sse64;
  }
  __syncthreads();
  if (tid == 0) {
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part_ssim[b] = (wave_ssim[0] + wave_ssim[1]) + (wave_ssim[2] + wave_ssim[3]);
    part_sse[b] = (wave_sse[0] + wave_sse[1]) + (wave_sse[2] + wave_sse[3]);
  }
}

// One workgroup: the partials of each plane in a fixed order -> the result record.
__global__ __launch_bounds__(256) void u8_metrics_finish_kernel(const double* __restrict__ part_ssim,
                                                                const unsigned long long* __restrict__ part_sse,
                                                                int per_plane, int planes, long long ssim_count,
                                                                long long n, unsigned long long* __restrict__ result) {
  __shared__ double sd[256];
  __shared__ unsigned long long se[256];
  const int tid = threadIdx.x;
  unsigned long long e = 0;
  for (int i = tid; i < per_plane * planes; i += 256) e += part_sse[i];
  se[tid] = e;
  for (int p = 0; p < 3; ++p) {
    double s = 0.0;
    if (p < planes)
      for (int i = tid; i < per_plane; i += 256) s += part_ssim[(size_t)p * per_plane + i];
    __syncthreads();
    sd[tid] = s;
    for (int o = 128; o > 0; o >>= 1) {
      __syncthreads();
      if (tid < o) {
        sd[tid] += sd[tid + o];
        if (p == 0) se[tid] += se[tid + o];
      }
    }
    if (tid == 0) result[1 + p] = (unsigned long long)__double_as_longlong(sd[0]);
  }
  if (tid == 0) {
    result[0] = se[0];
    result[4] = (unsigned long long)ssim_count;
    result[5] = (unsigned long long)n;
    result[6] = (unsigned long long)planes;
    result[7] = 0;
  }
}

struct MetricsGrid {
  int nx, ny, planes;
};

static inline bool metrics_shape_ok(int h, int w, int mode) {
  return h >= 1 && w >= 1 && h <= kMetMaxDim && w <= kMetMaxDim && (mode == 0 || mode == 1);
}

static inline MetricsGrid metrics_grid(int h, int w, int mode, bool ssim) {
  MetricsGrid g;
  g.planes = mode == 0 ? 3 : 1;
  if (ssim) {
    g.nx = (w - 2 * kMetR + kMetTX - 1) / kMetTX;
    g.ny = (h - 2 * kMetR + kMetTY - 1) / kMetTY;
  } else {
    g.nx = (w + kMetSX - 1) / kMetSX;
    g.ny = (h + kMetSY - 1) / kMetSY;
  }
  return g;
}

}  // namespace larva

using namespace larva;

extern "C" {

// Bytes of workspace larva_u8_metrics needs for a window of h x w (either value of want_ssim); -1 for a bad shape.
long long larva_u8_metrics_workspace_bytes(int h, int w, int mode) {
  if (!metrics_shape_ok(h, w, mode)) return -1;
  const MetricsGrid p = metrics_grid(h, w, mode, false);
  long long blocks = (long long)p.nx * p.ny;
  if (h >= kMetTaps && w >= kMetTaps) {
    const MetricsGrid s = metrics_grid(h, w, mode, true);
    blocks = std::max(blocks, (long long)s.nx * s.ny);
  }
  return blocks * p.planes * 16;
}

int larva_u8_metrics(const unsigned char* out, long long out_pitch, const unsigned char* truth, long long truth_pitch,
                     int y0, int x0, int h, int w, int mode, int want_ssim, void* workspace, unsigned long long* result,
                     void* stream) {
  if (!out || !truth || !workspace || !result || !metrics_shape_ok(h, w, mode) || y0 < 0 || x0 < 0 || y0 > kMetMaxDim ||
      x0 > kMetMaxDim || out_pitch < 3ll * (x0 + w) || truth_pitch < 3ll * (x0 + w) ||
      (want_ssim && (h < kMetTaps || w < kMetTaps)) || (reinterpret_cast<uintptr_t>(workspace) & 7u) ||
      (reinterpret_cast<uintptr_t>(result) & 7u))
    return (int)hipErrorInvalidValue;
  const MetricsGrid g = metrics_grid(h, w, mode, want_ssim != 0);
  const int per_plane = g.nx * g.ny;
  double* part_ssim = static_cast<double*>(workspace);
  unsigned long long* part_sse = reinterpret_cast<unsigned long long*>(workspace) + (size_t)per_plane * g.planes;
  GaussTaps taps;
  double sum = 0.0;
  for (int k = 0; k < kMetTaps; ++k) {
    const double d = (double)(k - kMetR);
    taps.w[k] = std::exp(-0.5 / (1.5 * 1.5) * d * d);
    sum += taps.w[k];
  }
  for (int k = 0; k < kMetTaps; ++k) taps.w[k] /= sum;
  const dim3 grid(g.nx, g.ny, g.planes), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0)
    hipLaunchKernelGGL((u8_metrics_kernel<0>), grid, block, 0, s, out, out_pitch, truth, truth_pitch, y0, x0, h, w,
                       want_ssim ? 1 : 0, taps, part_ssim, part_sse);
  else
    hipLaunchKernelGGL((u8_metrics_kernel<1>), grid, block, 0, s, out, out_pitch, truth, truth_pitch, y0, x0, h, w,
                       want_ssim ? 1 : 0, taps, part_ssim, part_sse);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const long long ssim_count = want_ssim ? (long long)(h - 2 * kMetR) * (w - 2 * kMetR) : 0;
  hipLaunchKernelGGL(u8_metrics_finish_kernel, dim3(1), dim3(256), 0, s, part_ssim, part_sse, per_plane, g.planes, ssim_count,
                     (long long)h * w * g.planes, result);
  return (int)hipGetLastError();
}

}  // extern "C"
