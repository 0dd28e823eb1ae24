// fp16 inference path (gfx950): 48-channel 3x3 convolutions on v_mfma_f32_16x16x32_f16, fp16 storage, fp32
// accumulation.  Only the grad-free x4 / 48-filter forward uses these kernels (larvanet_amd/half.py); training and the
// fp32 forward never reach them.
//
// Activations are fp16 CHANNELS-LAST, [N][H][W][48]: the 8 channels of one pixel's channel group are 16 contiguous
// bytes, the 8 K elements one lane feeds to the MFMA.  K is ordered (tap, 8-channel group): group g = 6 tap + cg,
// tap = 3 ky + kx, 54 groups = 13.5 K-steps of 32, padded to 14 (groups 54 and 55 are zero in the weight image, and
// their B fragments are forced to zero so that whatever the LDS holds there never reaches an accumulator).
//
// Conv GEMM per workgroup (256 threads, 4 waves): an output tile of 4 rows x 64 columns of one image.  Wave w owns row
// y0 + w, four 16-pixel N tiles, all 48 outputs (three 16-row M tiles): 12 accumulators of 4 floats.
//   A = weights  [cout][k]: the packed image (larva_f16_pack_weights) holds each lane's fragment of every (K-step,
//       M tile), [src][ks 14][m 3][lane 64][8 halves]; a wave loads all 42 fragments into registers once.
//   B = pixels   [k][pixel]: lane l reads group g = 4 ks + (l >> 4) of pixel (l & 15) + tap offset from the LDS halo.
//   C/D: lane l holds pixel (l & 15), outputs 16 m + 4 (l >> 4) + r, r = 0..3: four consecutive channels, one 8-byte
//       fp16 store (or, for the leg end, four consecutive HR pixels of one colour: one 16-byte fp32 store; its uint8
//       form gathers the lane's three colours of those pixels into 12 contiguous bytes of an HWC image).
// The input halo (6 rows x 66 columns x 48 channels) is staged in LDS with a pixel pitch of 112 bytes (7 slots of
// 16 B, coprime to the 16 slots of a bank row), so 16 consecutive pixels of a ds_read_b128 hit 16 distinct slots.
// A multi-source conv (the V2 merge conv over M body outputs, no concatenation) repeats weights + halo + 14 K-steps
// per source, accumulating into the same registers.
//
// Every pixel's sum is the same sequence of MFMAs over the same K order whatever tile, batch position or image height
// it falls into, so results are bit-identical across tilings, bands and batch sizes.
//
// Job launches (conv_jobs_kernel): 1..8 independent single-source convs of one shape in one grid -- the legs of a multi-exit
// network, which depend on the bodies and not on each other.  A workgroup looks its job up from blockIdx.x and then runs
// conv_tile, the one tile body the single-job kernels run, so job j is bit for bit the single-job launch of its operands.
// Block b is tile 8 (b / (8 njobs)) + b % 8 of job (b / 8) % njobs: the job index sits between a group of eight tiles and
// the groups.  Blocks are dealt to the eight XCDs round-robin (observed, relied on for speed only), so b and b + 8 share an
// L2: the njobs workgroups that read one tile of the shared base image are 8 apart, on one L2 and dispatched together,
// while the eight neighbouring tiles of one job, which share halo rows of that job's source, stay next to each other as
// in the single-job grid.  Sources and weights are per job and gain nothing from either order.  The grid is padded to
// whole groups; a workgroup whose tile does not exist leaves at once.
//
// Overflow: an epilogue that stores fp16 sets *flag = 1 (a plain vector store; every writer stores the same value)
// when the pre-activation value is not finite, or the stored value is not finite or exceeds 65504 in magnitude.  The
// pre-activation test catches a NaN that the ReLU would otherwise turn into 0.  The uint8 leg end sets it when the fp32
// value it is about to quantise is not finite (the fp32 leg end stores that value as it is).
#include <stdint.h>

#include "larva_common.h"

namespace larva {
namespace f16 {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kC = 48;                        // channels of every fp16 activation
constexpr int kGroups = 54;                   // 9 taps x 6 groups of 8 channels
constexpr int kKSteps = 14;                   // ceil(54 / 4)
constexpr int kMT = 3;                        // 16-output M tiles
constexpr int kRows = 4;                      // output rows per workgroup (one per wave)
constexpr int kNT = 4;                        // 16-pixel N tiles per wave
constexpr int kCols = kNT * 16;               // output columns per workgroup
constexpr int kHR = kRows + 2, kHC = kCols + 2;
constexpr int kPix16 = 7;                     // LDS pitch of one halo pixel, in 16-byte slots (6 used)
constexpr int kHaloSlots = kHR * kHC * kPix16;
constexpr int kFragsPerSrc = kKSteps * kMT * 64;   // 16-byte fragments of the weight image per source
constexpr int kMaxSrc = 8;
constexpr float kHalfMax = 65504.f;

enum Epi { EPI_BIAS = 0, EPI_RELU = 1, EPI_RES0 = 2, EPI_RES01 = 3, EPI_SHUFFLE = 4, EPI_SHUFFLE_U8 = 5 };

struct ConvArgs {
  const uint16_t* src[kMaxSrc];
  int nsrc;
  const uint16_t* wpk;
  const float* bias;
  const uint16_t* res0;
  const uint16_t* res1;
  uint16_t* out;           // fp16 [N][H][W][48]            (EPI_BIAS .. EPI_RES01)
  const float* base;       // fp32 [N][3][4H][4W]           (EPI_SHUFFLE, EPI_SHUFFLE_U8)
  float* out_hr;           // fp32 [N][3][4H][4W]           (EPI_SHUFFLE)
  unsigned* flag;
  int H, W, tiles_x, tiles_y;
  unsigned char* out_u8;   // uint8 [N][4H][4W][3]          (EPI_SHUFFLE_U8)
};

constexpr int kMaxJobs = 8;

struct JobArgs {
  const uint16_t* src[kMaxJobs];
  const uint16_t* wpk[kMaxJobs];
  const float* bias[kMaxJobs];
  void* out[kMaxJobs];     // fp16 [N][H][W][48] (EPI_BIAS, EPI_RELU), fp32 [N][3][4H][4W] (EPI_SHUFFLE), uint8 [N][4H][4W][3]
  const float* base;       // fp32 [N][3][4H][4W], shared by every job
  unsigned* flag;
  int njobs, H, W, tiles_x, tiles_y, tiles;   // tiles = N tiles_y tiles_x of ONE job
};

// One job of a JobArgs as conv_tile reads it: ConvArgs' member names, one source.
struct JobView {
  const uint16_t* src[1];
  static constexpr int nsrc = 1;
  const uint16_t* wpk;
  const float* bias;
  static constexpr const uint16_t* res0 = nullptr;
  static constexpr const uint16_t* res1 = nullptr;
  uint16_t* out;
  const float* base;
  float* out_hr;
  unsigned* flag;
  int H, W, tiles_x, tiles_y;
  unsigned char* out_u8;
};

__device__ __forceinline__ h8 as_h8(uint4 v) { return __builtin_bit_cast(h8, v); }

// One output tile: tile t of the N x tiles_y x tiles_x tiles of the conv `a` describes (a ConvArgs, or one job's JobView).
template <int EPI, class Args>
__device__ __forceinline__ void conv_tile(const Args& a, int t) {
  __shared__ uint4 halo[kHaloSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hq = lane >> 4, col = lane & 15;
  const int tx = t % a.tiles_x;
  t /= a.tiles_x;
  const int ty = t % a.tiles_y;
  const int n = t / a.tiles_y;
  const int x0 = tx * kCols, y0 = ty * kRows;
  const int H = a.H, W = a.W;

  f4 acc[kMT][kNT];
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) acc[m][nt] = f4{0.f, 0.f, 0.f, 0.f};

  for (int s = 0; s < a.nsrc; ++s) {
    h8 wa[kKSteps][kMT];
    const uint4* wp = reinterpret_cast<const uint4*>(a.wpk) + (size_t)s * kFragsPerSrc + lane;
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks)
#pragma unroll
      for (int m = 0; m < kMT; ++m) wa[ks][m] = as_h8(wp[(ks * kMT + m) * 64]);

    if (s) __syncthreads();   // every wave is done reading the previous source's halo
    const uint16_t* src = a.src[s];
    for (int c = tid; c < kHR * kHC * 6; c += 256) {
      const int r = c / (kHC * 6), rem = c - r * (kHC * 6), px = rem / 6, ch = rem - px * 6;
      const int yy = y0 - 1 + r, xx = x0 - 1 + px;
      uint4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
        v = *reinterpret_cast<const uint4*>(src + (((size_t)n * H + yy) * W + xx) * kC + ch * 8);
      halo[(r * kHC + px) * kPix16 + ch] = v;
    }
    __syncthreads();

#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) {
      const bool valid = ks < kKSteps - 1 || hq < 2;   // group 4 ks + hq < 54
      const int g = valid ? 4 * ks + hq : 0;
      const int tap = g / 6, cg = g - 6 * tap, dy = tap / 3, dx = tap - 3 * dy;
      const int b0 = ((wave + dy) * kHC + col + dx) * kPix16 + cg;
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt) {
        if (x0 + nt * 16 >= W) continue;   // (wave-uniform: a tile past the image's right edge)
        uint4 bv = halo[b0 + nt * 16 * kPix16];
        if (!valid) bv = uint4{0u, 0u, 0u, 0u};
        const h8 b = as_h8(bv);
#pragma unroll
        for (int m = 0; m < kMT; ++m) acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[ks][m], b, acc[m][nt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue
  const int y = y0 + wave;
  if (y >= H) return;
  bool bad = false;
#pragma unroll
  for (int nt = 0; nt < kNT; ++nt) {
    const int x = x0 + nt * 16 + col;
    if (x >= W) continue;
    const size_t pix = ((size_t)n * H + y) * W + x;
    f4 rgb[kMT];   // (EPI_SHUFFLE_U8: the three colours of this lane's four HR pixels)
#pragma unroll
    for (int m = 0; m < kMT; ++m) {
      const int c0 = 16 * m + 4 * hq;
      const f4 bias = *reinterpret_cast<const f4*>(a.bias + c0);
      f4 v = acc[m][nt] + bias;
      if constexpr (EPI == EPI_SHUFFLE) {
        // PixelShuffle(4): channel 16 m + 4 hq + r -> colour m, HR row 4 y + hq, HR column 4 x + r
        const size_t o = (((size_t)n * 3 + m) * (4 * H) + 4 * y + hq) * (size_t)(4 * W) + 4 * (size_t)x;
        const f4 bs = *reinterpret_cast<const f4*>(a.base + o);
        *reinterpret_cast<f4*>(a.out_hr + o) = v + bs;
      } else if constexpr (EPI == EPI_SHUFFLE_U8) {
        // the same fp32 value EPI_SHUFFLE stores; a non-finite one raises the flag instead of becoming a byte silently
        const size_t o = (((size_t)n * 3 + m) * (4 * H) + 4 * y + hq) * (size_t)(4 * W) + 4 * (size_t)x;
        const f4 bs = *reinterpret_cast<const f4*>(a.base + o);
        rgb[m] = v + bs;
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= !__builtin_isfinite(rgb[m][r]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= !__builtin_isfinite(v[r]);
        if constexpr (EPI == EPI_RELU) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if constexpr (EPI == EPI_RES0 || EPI == EPI_RES01) {
          const h4 r0 = *reinterpret_cast<const h4*>(a.res0 + pix * kC + c0);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)r0[r];
        }
        if constexpr (EPI == EPI_RES01) {
          const h4 r1 = *reinterpret_cast<const h4*>(a.res1 + pix * kC + c0);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)r1[r];
        }
        h4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          bad |= !(fabsf(v[r]) <= kHalfMax);
          o[r] = (_Float16)v[r];
        }
        *reinterpret_cast<h4*>(a.out + pix * kC + c0) = o;
      }
    }
    if constexpr (EPI == EPI_SHUFFLE_U8) {
      // R, G, B of HR row 4 y + hq, HR columns 4 x .. 4 x + 3: 12 contiguous bytes of the HWC image (192 per quarter-wave)
      const size_t o = (((size_t)n * (4 * H) + 4 * y + hq) * (size_t)(4 * W) + 4 * (size_t)x) * 3;
      *reinterpret_cast<rgb4_bytes*>(a.out_u8 + o) = pack_rgb4(rgb[0], rgb[1], rgb[2]);
    }
  }
  if (bad) *a.flag = 1u;
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void conv_kernel(ConvArgs a) {
  conv_tile<EPI>(a, (int)blockIdx.x);
}

// 1..8 single-source convs of one shape in one grid (see the header comment for the block order).  The job and the tile
// are uniform over the workgroup, so the job's pointers are scalar loads from the kernel arguments.
template <int EPI>
__global__ __launch_bounds__(256, 2) void conv_jobs_kernel(JobArgs a) {
  const unsigned b = blockIdx.x, group = b / (8u * (unsigned)a.njobs);
  const int job = (int)((b >> 3) - group * (unsigned)a.njobs);
  const int t = (int)(group * 8u + (b & 7u));
  if (t >= a.tiles) return;   // (the padding of the last group of eight)
  JobView v = {};
  v.src[0] = a.src[job];
  v.wpk = a.wpk[job];
  v.bias = a.bias[job];
  v.base = a.base;
  v.flag = a.flag;
  v.H = a.H;
  v.W = a.W;
  v.tiles_x = a.tiles_x;
  v.tiles_y = a.tiles_y;
  if constexpr (EPI == EPI_SHUFFLE) v.out_hr = static_cast<float*>(a.out[job]);
  else if constexpr (EPI == EPI_SHUFFLE_U8) v.out_u8 = static_cast<unsigned char*>(a.out[job]);
  else v.out = static_cast<uint16_t*>(a.out[job]);
  conv_tile<EPI>(v, t);
}

// Head: fp32 NCHW image (3 channels) -> fp16 [N][H][W][48], + bias.  fp32 VALU form: fp32 operands (the image and the
// fp32 weights, not rounded to fp16), fp32 fmaf chain over k = (cin, ky, kx) in PyTorch's weight order, + bias, then
// one rounding to fp16.  One thread per (pixel, 16-output group); blockIdx.y is the group, so the weights are
// wave-uniform.
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                   const float* __restrict__ b, uint16_t* __restrict__ out,
                                                   unsigned* flag, int N, int H, int W) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)N * H * W) return;
  const int xx = (int)(p % W);
  const long long t = p / W;
  const int yy = (int)(t % H), n = (int)(t / H);
  float in[27];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int y = yy + ky - 1, xc = xx + kx - 1;
        const bool in_img = (unsigned)y < (unsigned)H && (unsigned)xc < (unsigned)W;
        in[(c * 3 + ky) * 3 + kx] = in_img ? x[(((size_t)n * 3 + c) * H + y) * W + xc] : 0.f;
      }
  const int g = blockIdx.y;
  bool bad = false;
  h8 o[2];
#pragma unroll
  for (int co = 0; co < 16; ++co) {
    const float* wr = w + (size_t)(16 * g + co) * 27;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc = fmaf(wr[k], in[k], acc);
    const float v = acc + b[16 * g + co];
    bad |= !(fabsf(v) <= kHalfMax);
    o[co >> 3][co & 7] = (_Float16)v;
  }
  h8* dst = reinterpret_cast<h8*>(out + (size_t)p * kC + 16 * g);
  dst[0] = o[0];
  dst[1] = o[1];
  if (bad) *flag = 1u;
}

// [48][48 nsrc][3][3] fp32 -> the A-fragment image [src][ks][m][lane][8] fp16 (round to nearest even).
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int nsrc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nsrc * kFragsPerSrc) return;
  const int lane = i & 63, t = i >> 6;
  const int m = t % kMT, ks = (t / kMT) % kKSteps, s = t / (kMT * kKSteps);
  const int cout = 16 * m + (lane & 15), g = 4 * ks + (lane >> 4);
  const int cin_total = kC * nsrc;
  h8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = 0.f;
    if (g < kGroups) {
      const int tap = g / 6, cg = g - 6 * tap;
      f = w[((size_t)cout * cin_total + s * kC + cg * 8 + j) * 9 + tap];
    }
    v[j] = (_Float16)f;
  }
  reinterpret_cast<h8*>(out)[i] = v;
}

static long long tiles_of(int N, int H, int W) {
  return (long long)N * ((H + kRows - 1) / kRows) * ((W + kCols - 1) / kCols);
}

// njobs > 1: the grid of a job launch, njobs times the tiles rounded up to whole groups of eight, must fit as well
static bool shape_ok(int N, int H, int W, int njobs = 1) {
  return N > 0 && H > 0 && W > 0 && (long long)N * H * W * kC < (1ll << 40) &&
         (tiles_of(N, H, W) + 7) / 8 * 8 * njobs < (1ll << 31);
}

// What the kernels access wide, and so what the launchers refuse (hipErrorInvalidValue) before anything is launched:
// fp16 activations (sources, residuals, outputs), packed weight images, the conv kernels' fp32 bias, the fp32 base and
// HR output images are moved 16 bytes at a time (a residual and a conv output 8, held to the same rule: an output is the
// next layer's source); the uint8 HR image is written as three 4-byte words per lane.  The head's image, weights and
// bias and the overflow flag are accessed one element at a time: any address their type allows.
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

static bool conv_ptrs_ok(const ConvArgs& a) {
  for (int i = 0; i < a.nsrc; ++i)
    if (!aligned16(a.src[i])) return false;
  return aligned16(a.wpk) && aligned16(a.bias) && aligned16(a.res0) && aligned16(a.res1) && aligned16(a.out) &&
         aligned16(a.base) && aligned16(a.out_hr) && aligned4(a.out_u8);
}

static int launch_conv(int epi, ConvArgs& a, int N, hipStream_t s) {
  if (!conv_ptrs_ok(a)) return (int)hipErrorInvalidValue;
  a.tiles_x = (a.W + kCols - 1) / kCols;
  a.tiles_y = (a.H + kRows - 1) / kRows;
  const dim3 grid((unsigned)((long long)N * a.tiles_x * a.tiles_y)), block(256);
  switch (epi) {
    case EPI_BIAS: hipLaunchKernelGGL(conv_kernel<EPI_BIAS>, grid, block, 0, s, a); break;
    case EPI_RELU: hipLaunchKernelGGL(conv_kernel<EPI_RELU>, grid, block, 0, s, a); break;
    case EPI_RES0: hipLaunchKernelGGL(conv_kernel<EPI_RES0>, grid, block, 0, s, a); break;
    case EPI_RES01: hipLaunchKernelGGL(conv_kernel<EPI_RES01>, grid, block, 0, s, a); break;
    case EPI_SHUFFLE_U8: hipLaunchKernelGGL(conv_kernel<EPI_SHUFFLE_U8>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(conv_kernel<EPI_SHUFFLE>, grid, block, 0, s, a); break;
  }
  return (int)hipGetLastError();
}

// The common part of the two job entry points: argument checks, then one launch.  outs are the njobs output images of
// the epilogue `epi`; base and flag may be NULL where the epilogue does not use them (the callers have checked).
static int launch_jobs(int epi, int njobs, const uint16_t* const* srcs, const uint16_t* const* wpks,
                       const float* const* biases, void* const* outs, const float* base, unsigned* flag, int N, int H,
                       int W, hipStream_t s) {
  if (njobs < 1 || njobs > kMaxJobs || !srcs || !wpks || !biases || !outs || !shape_ok(N, H, W, njobs))
    return (int)hipErrorInvalidValue;
  if (!aligned16(base)) return (int)hipErrorInvalidValue;
  JobArgs a = {};
  for (int j = 0; j < njobs; ++j) {
    if (!srcs[j] || !wpks[j] || !biases[j] || !outs[j]) return (int)hipErrorInvalidValue;
    if (!aligned16(srcs[j]) || !aligned16(wpks[j]) || !aligned16(biases[j]) ||
        !(epi == EPI_SHUFFLE_U8 ? aligned4(outs[j]) : aligned16(outs[j])))
      return (int)hipErrorInvalidValue;
    a.src[j] = srcs[j];
    a.wpk[j] = wpks[j];
    a.bias[j] = biases[j];
    a.out[j] = outs[j];
  }
  a.base = base;
  a.flag = flag;
  a.njobs = njobs;
  a.H = H;
  a.W = W;
  a.tiles_x = (W + kCols - 1) / kCols;
  a.tiles_y = (H + kRows - 1) / kRows;
  a.tiles = (int)tiles_of(N, H, W);
  const dim3 grid((unsigned)((tiles_of(N, H, W) + 7) / 8 * 8 * njobs)), block(256);
  switch (epi) {
    case EPI_BIAS: hipLaunchKernelGGL(conv_jobs_kernel<EPI_BIAS>, grid, block, 0, s, a); break;
    case EPI_RELU: hipLaunchKernelGGL(conv_jobs_kernel<EPI_RELU>, grid, block, 0, s, a); break;
    case EPI_SHUFFLE_U8: hipLaunchKernelGGL(conv_jobs_kernel<EPI_SHUFFLE_U8>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(conv_jobs_kernel<EPI_SHUFFLE>, grid, block, 0, s, a); break;
  }
  return (int)hipGetLastError();
}

}  // namespace f16
}  // namespace larva

using namespace larva::f16;

extern "C" {

long long larva_f16_packed_weight_halves(int cout, int cin) {
  if (cout != kC || cin <= 0 || cin % kC || cin / kC > kMaxSrc) return -1;
  return (long long)(cin / kC) * kFragsPerSrc * 8;
}

int larva_f16_pack_weights(const float* w, uint16_t* wpk, int cout, int cin, void* stream) {
  const long long halves = larva_f16_packed_weight_halves(cout, cin);
  if (!w || !wpk || halves < 0 || !aligned16(wpk)) return (int)hipErrorInvalidValue;
  const int frags = (int)(halves / 8);
  hipLaunchKernelGGL(pack_kernel, dim3((frags + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, wpk, cin / kC);
  return (int)hipGetLastError();
}

int larva_f16_head(const float* x, const float* w, const float* bias, uint16_t* out, unsigned* flag, int N, int H,
                   int W, void* stream) {
  if (!x || !w || !bias || !out || !flag || !shape_ok(N, H, W) || !aligned16(out)) return (int)hipErrorInvalidValue;
  const long long px = (long long)N * H * W;
  hipLaunchKernelGGL(head_kernel, dim3((unsigned)((px + 255) / 256), 3), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                     out, flag, N, H, W);
  return (int)hipGetLastError();
}

int larva_f16_conv3x3(const uint16_t* const* srcs, int nsrc, const uint16_t* wpk, const float* bias,
                      const uint16_t* res0, const uint16_t* res1, int relu, uint16_t* out, unsigned* flag, int N, int H,
                      int W, void* stream) {
  if (!srcs || nsrc < 1 || nsrc > kMaxSrc || !wpk || !bias || !out || !flag || !shape_ok(N, H, W) ||
      (res1 && !res0) || (relu && res0))
    return (int)hipErrorInvalidValue;
  ConvArgs a = {};
  for (int i = 0; i < nsrc; ++i) {
    if (!srcs[i]) return (int)hipErrorInvalidValue;
    a.src[i] = srcs[i];
  }
  a.nsrc = nsrc;
  a.wpk = wpk;
  a.bias = bias;
  a.res0 = res0;
  a.res1 = res1;
  a.out = out;
  a.flag = flag;
  a.H = H;
  a.W = W;
  const int epi = res1 ? EPI_RES01 : res0 ? EPI_RES0 : relu ? EPI_RELU : EPI_BIAS;
  return launch_conv(epi, a, N, (hipStream_t)stream);
}

int larva_f16_conv3x3_shuffle_base(const uint16_t* src, const uint16_t* wpk, const float* bias, const float* base,
                                   float* out, int N, int H, int W, void* stream) {
  if (!src || !wpk || !bias || !base || !out || !shape_ok(N, H, W)) return (int)hipErrorInvalidValue;
  ConvArgs a = {};
  a.src[0] = src;
  a.nsrc = 1;
  a.wpk = wpk;
  a.bias = bias;
  a.base = base;
  a.out_hr = out;
  a.H = H;
  a.W = W;
  return launch_conv(EPI_SHUFFLE, a, N, (hipStream_t)stream);
}

int larva_f16_conv3x3_shuffle_base_u8(const uint16_t* src, const uint16_t* wpk, const float* bias, const float* base,
                                      unsigned char* out, unsigned* flag, int N, int H, int W, void* stream) {
  if (!src || !wpk || !bias || !base || !out || !flag || !shape_ok(N, H, W)) return (int)hipErrorInvalidValue;
  ConvArgs a = {};
  a.src[0] = src;
  a.nsrc = 1;
  a.wpk = wpk;
  a.bias = bias;
  a.base = base;
  a.out_u8 = out;
  a.flag = flag;
  a.H = H;
  a.W = W;
  return launch_conv(EPI_SHUFFLE_U8, a, N, (hipStream_t)stream);
}

int larva_f16_conv3x3_jobs(int njobs, const uint16_t* const* srcs, const uint16_t* const* wpks,
                           const float* const* biases, int relu, uint16_t* const* outs, unsigned* flag, int N, int H,
                           int W, void* stream) {
  if (!flag) return (int)hipErrorInvalidValue;
  return launch_jobs(relu ? EPI_RELU : EPI_BIAS, njobs, srcs, wpks, biases, reinterpret_cast<void* const*>(outs), nullptr,
                     flag, N, H, W, (hipStream_t)stream);
}

int larva_f16_conv3x3_shuffle_base_jobs(int njobs, const uint16_t* const* srcs, const uint16_t* const* wpks,
                                        const float* const* biases, const float* base, float* const* outs_f32,
                                        unsigned char* const* outs_u8, unsigned* flag, int N, int H, int W,
                                        void* stream) {
  if (!base || (outs_f32 != nullptr) == (outs_u8 != nullptr) || (outs_u8 && !flag)) return (int)hipErrorInvalidValue;
  return launch_jobs(outs_u8 ? EPI_SHUFFLE_U8 : EPI_SHUFFLE, njobs, srcs, wpks, biases,
                     outs_u8 ? reinterpret_cast<void* const*>(outs_u8) : reinterpret_cast<void* const*>(outs_f32), base,
                     flag, N, H, W, (hipStream_t)stream);
}

}  // extern "C"
