// Geometric self-ensemble (x8) around the inference forward (gfx950): the eight flips / transposes of the input
// image as batch slots, and the inverse transform + mean (+ quantise) of the eight fp32 HR results in one launch.
//
// dihedral(a, t) over the spatial axes (r, c), t = 0..7: reverse rows if t & 1, then reverse columns if t & 2, then
// swap the axes if t & 4 (image_utils.dihedral).  With fr(r) = t & 1 ? H - 1 - r : r and fc(c) = t & 2 ? W - 1 - c : c:
//     t < 4:   x_t [H][W],  x_t[r][c] = x[fr(r)][fc(c)]        -> slot 4 n + t     of A [4N][3][H][W]
//     t >= 4:  x_t [W][H],  x_t[i][j] = x[fr(j)][fc(i)]        -> slot 4 n + t - 4 of B [4N][3][W][H]
// The forward maps A -> A' [4N][3][sH][sW] and B -> B' [4N][3][sW][sH]; mapped back (dihedral_inv), at HR sizes,
//     t < 4:   v_t[y][x] = A'_t[fr(y)][fc(x)]          t >= 4:  v_t[y][x] = B'_t[fc(x)][fr(y)]
// and E = (((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125f for every pixel, in this order, whatever the
// tile; the uint8 form is quantize_u8(E) as HWC bytes = larva_f32_chw_to_u8_hwc of the float form.
//
// Both kernels work on 32 x 32 tiles with 256 threads and move the transposed operands through an LDS tile of pitch
// 33 floats: the tile is written along one axis and read along the other, both as ds_write_b32 / ds_read_b32 (banks
// (a / 4) mod 32 per 32-lane half).  In the merge a half-wave writes rows xi = l >> 3 at columns 4 (l & 7) + k: bank
// (xi + 4 (l & 7) + k) mod 32, 32 distinct values; it reads rows 4 (l & 7) + k at column l >> 3: bank (4 (l & 7) + k
// + (l >> 3)) mod 32, again distinct.  A pitch of 36 would allow 16-byte LDS accesses on one side and cost a 4-way
// conflict on the other.  Flips only reverse the order inside a lane's 4 pixels and of the lanes: no staging.
#include "larva_common.h"

namespace larva {

constexpr int kEnsTile = 32;
constexpr int kEnsPitch = kEnsTile + 1;

__device__ __forceinline__ float as_float(unsigned char v) { return (float)v; }
__device__ __forceinline__ float as_float(float v) { return v; }

// ---------------------------------------------------------------------------------------------
// The eight inputs.  src: uint8 [N][H][W][3] (T = unsigned char) or float [N][3][H][W] (T = float).  A workgroup reads
// one 32 x 32 tile of one image once (all three colours) into LDS and writes it eight times: the four flips row by
// row as it was read, the four transposes with the roles of the thread indices swapped, so that a wave's stores are
// contiguous runs of B's rows as well.  Block (32, 8), grid (ceil(W / 32), ceil(H / 32), N).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dihedral_inputs_kernel(const T* __restrict__ src, float* __restrict__ A,
                                                              float* __restrict__ B, int H, int W) {
  __shared__ float tile[3][kEnsTile * kEnsPitch];
  const int n = blockIdx.z, r0 = blockIdx.y * kEnsTile, c0 = blockIdx.x * kEnsTile;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int lr = ty + 8 * k, r = r0 + lr, c = c0 + tx;
    if (r < H && c < W) {
      const size_t px = (size_t)r * W + c;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float v;
        if constexpr (sizeof(T) == 1) v = as_float(src[((size_t)n * plane + px) * 3 + ch]);
        else v = as_float(src[((size_t)n * 3 + ch) * plane + px]);
        tile[ch][lr * kEnsPitch + tx] = v;
      }
    }
  }
  __syncthreads();
  float* a = A + (size_t)(4 * n) * 3 * plane;
  float* b = B + (size_t)(4 * n) * 3 * plane;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // flips: x_t[fr(r)][fc(c)] = x[r][c] (fr, fc are involutions); tx runs along the columns
    const int lr = ty + 8 * k, r = r0 + lr, c = c0 + tx;
    if (r < H && c < W) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float v = tile[ch][lr * kEnsPitch + tx];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int rr = (t & 1) ? H - 1 - r : r, cc = (t & 2) ? W - 1 - c : c;
          a[((size_t)t * 3 + ch) * plane + (size_t)rr * W + cc] = v;
        }
      }
    }
    // transposes: x_t[fc(c)][fr(r)] = x[r][c]; tx runs along the source rows = B's columns
    const int lc = ty + 8 * k, c2 = c0 + lc, r2 = r0 + tx;
    if (r2 < H && c2 < W) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float v = tile[ch][tx * kEnsPitch + lc];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int jj = (t & 1) ? H - 1 - r2 : r2, ii = (t & 2) ? W - 1 - c2 : c2;
          b[((size_t)t * 3 + ch) * plane + (size_t)ii * H + jj] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Four logical positions p .. p + 3 of an axis of length L along `line`, the axis reversed when rev: element k is
// line[rev ? L - 1 - p - k : p + k], 0 where p + k >= L.  VEC: L % 4 == 0, p % 4 == 0 and `line` 16-byte aligned, so
// the run is whole or absent and one 16-byte load fetches it.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ f32x4 load_run(const float* __restrict__ line, int p, int L, bool rev) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    if (p < L) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(line + (rev ? L - 4 - p : p));
      v = rev ? f32x4{u[3], u[2], u[1], u[0]} : u;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (p + k < L) v[k] = line[rev ? L - 1 - p - k : p + k];
  }
  return v;
}

// ---------------------------------------------------------------------------------------------
// The merge.  A [4N][3][H][W], B [4N][3][W][H] (H, W: the HR sizes) -> E float [N][3][H][W] or uint8 [N][H][W][3].  A
// workgroup owns 32 x 32 pixels of one image; thread (row = tid >> 3, q = tid & 7) owns pixels (y0 + row, x0 + 4 q ..
// + 3) of all three colours.  Per colour it loads its four A operands (8 lanes = 128 contiguous bytes of a row) and,
// in the other role (row -> E column x0 + row = one row of B', q -> E rows y0 + 4 q .. + 3 = 4 consecutive floats of
// that row), one run of each of the four B' operands into LDS; after the barrier it reads its own pixels' B' values
// across the tile.  Nothing but E is stored.  The sum is the fixed chain of adds (no contraction: there is no
// multiply in front of an add), `* 0.125f` is exact.
// ---------------------------------------------------------------------------------------------
template <bool VEC, bool U8>
__global__ __launch_bounds__(256) void dihedral_mean_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                            void* __restrict__ out, int H, int W) {
#pragma clang fp contract(off)
  __shared__ float tile[4][kEnsTile * kEnsPitch];
  const int n = blockIdx.z, y0 = blockIdx.y * kEnsTile, x0 = blockIdx.x * kEnsTile;
  const int tid = threadIdx.x, q = tid & 7, row = tid >> 3;
  const int y = y0 + row, x = x0 + 4 * q;     // this thread's pixels
  const int bx = x0 + row, by = y0 + 4 * q;   // the run of B' it stages
  const size_t plane = (size_t)H * W;
  f32x4 acc[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* a = A + ((size_t)(4 * n) * 3 + ch) * plane;
    const float* b = B + ((size_t)(4 * n) * 3 + ch) * plane;
    if (ch) __syncthreads();   // the previous colour's tile has been read
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 u = {0.f, 0.f, 0.f, 0.f};
      if (bx < W) u = load_run<VEC>(b + (size_t)t * 3 * plane + (size_t)((t & 2) ? W - 1 - bx : bx) * H, by, H, t & 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) tile[t][row * kEnsPitch + 4 * q + k] = u[k];
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (y < H) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 v = load_run<VEC>(a + (size_t)t * 3 * plane + (size_t)((t & 1) ? H - 1 - y : y) * W, x, W, t & 2);
        s = t == 0 ? v : s + v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = tile[t][(4 * q + k) * kEnsPitch + row];
      s = s + v;
    }
    acc[ch] = s * 0.125f;
  }
  if (y >= H || x >= W) return;
  if constexpr (U8) {
    unsigned char* o = static_cast<unsigned char*>(out) + (((size_t)n * H + y) * W + x) * 3;
    if constexpr (VEC) {   // 12 contiguous bytes at a multiple of 12
      *reinterpret_cast<rgb4_bytes*>(o) = pack_rgb4(acc[0], acc[1], acc[2]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) o[3 * k + ch] = (unsigned char)quantize_u8(acc[ch][k]);
        }
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float* o = static_cast<float*>(out) + ((size_t)n * 3 + ch) * plane + (size_t)y * W + x;
      if constexpr (VEC) {
        *reinterpret_cast<f32x4*>(o) = acc[ch];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x + k < W) o[k] = acc[ch][k];
      }
    }
  }
}

static bool ens_shape_ok(int N, int H, int W) {
  // grid.z = N, grid.y = ceil(H / 32): both below 65536
  return N > 0 && N < 65536 && H > 0 && W > 0 && H <= (1 << 20) && W <= (1 << 20) &&
         (long long)N * H * W * 12 < (1ll << 40);
}

template <typename T>
static int launch_inputs(const T* in, float* a, float* b, int N, int H, int W, void* stream) {
  if (!in || !a || !b || !ens_shape_ok(N, H, W)) return (int)hipErrorInvalidValue;
  const dim3 grid((W + kEnsTile - 1) / kEnsTile, (H + kEnsTile - 1) / kEnsTile, N), block(kEnsTile, 8);
  hipLaunchKernelGGL(dihedral_inputs_kernel<T>, grid, block, 0, (hipStream_t)stream, in, a, b, H, W);
  return (int)hipGetLastError();
}

}  // namespace larva

using namespace larva;

extern "C" {

// a [4N][3][H][W], b [4N][3][W][H] = the eight dihedral images of in uint8 [N][H][W][3], exact.
int larva_dihedral_inputs_u8(const unsigned char* in, float* a, float* b, int N, int H, int W, void* stream) {
  return launch_inputs(in, a, b, N, H, W, stream);
}

// The same of in float [N][3][H][W].
int larva_dihedral_inputs_f32(const float* in, float* a, float* b, int N, int H, int W, void* stream) {
  return launch_inputs(in, a, b, N, H, W, stream);
}

// a [4N][3][H][W], b [4N][3][W][H] -> the mean of the eight images mapped back, into out_f32 [N][3][H][W] or out_u8
// [N][H][W][3] (exactly one of them given).
int larva_dihedral_mean(const float* a, const float* b, float* out_f32, unsigned char* out_u8, int N, int H, int W,
                        void* stream) {
  if (!a || !b || (out_f32 == nullptr) == (out_u8 == nullptr) || !ens_shape_ok(N, H, W)) return (int)hipErrorInvalidValue;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                         reinterpret_cast<uintptr_t>(out_f32) | reinterpret_cast<uintptr_t>(out_u8);
  const bool vec = H % 4 == 0 && W % 4 == 0 && (bits & 15u) == 0;
  const dim3 grid((W + kEnsTile - 1) / kEnsTile, (H + kEnsTile - 1) / kEnsTile, N), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (out_u8) {
    if (vec) hipLaunchKernelGGL((dihedral_mean_kernel<true, true>), grid, block, 0, s, a, b, (void*)out_u8, H, W);
    else hipLaunchKernelGGL((dihedral_mean_kernel<false, true>), grid, block, 0, s, a, b, (void*)out_u8, H, W);
  } else {
    if (vec) hipLaunchKernelGGL((dihedral_mean_kernel<true, false>), grid, block, 0, s, a, b, (void*)out_f32, H, W);
    else hipLaunchKernelGGL((dihedral_mean_kernel<false, false>), grid, block, 0, s, a, b, (void*)out_f32, H, W);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
